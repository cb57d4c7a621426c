"""The host orchestration (qwen_tts.c) against a recording fake device, on a CPU.

tests/host_trace/driver.c runs every public generate path against
tests/host_trace/fake_dev.c, which implements the device C-ABI of
include/qtts_hip.h deterministically and logs every call.  The program is built
here with AddressSanitizer and UBSan as a stand-alone executable.

 - every scenario's trace (device calls with their arguments, return values,
   output and callback hashes, last_* / queue_*) equals its fixture in
   tests/golden/host_trace/ byte for byte: the fixtures were recorded from the
   host code before the prompt / stream / codec helpers were shared;
 - the fault sweep: for every K up to the scenario's device calls, the run with
   the K-th call failing leaves no dangling or inconsistent output, consumes both
   armings, is followed by a clean generate that reproduces its trace, and the
   process ends with the sanitizers (LeakSanitizer included) silent.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qwen3-tts-c_amd", "csrc", "host")
SRC = os.path.join(HERE, "host_trace")
FIXTURES = os.path.join(HERE, "golden", "host_trace")
SCENARIOS = sorted(f[:-len(".trace")] for f in os.listdir(FIXTURES) if f.endswith(".trace"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_trace") / "driver")
    srcs = [os.path.join(SRC, "driver.c"), os.path.join(SRC, "fake_dev.c")]
    srcs += [os.path.join(HOST, f) for f in ("qwen_tts.c", "qjson.c", "wav.c", "bpe.c")]
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, *srcs, "-lm"], check=True)
    return exe


def _run(exe, model, mode, name):
    return subprocess.run([exe, model, mode, name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=120)


def test_every_scenario_has_a_fixture_and_the_other_way_round(driver, tiny_dir):
    listed = subprocess.run([driver, tiny_dir, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert sorted(listed) == SCENARIOS


@pytest.mark.parametrize("name", SCENARIOS)
def test_trace_equals_the_fixture(driver, tiny_dir, name):
    r = _run(driver, tiny_dir, "--trace", name)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(os.path.join(FIXTURES, name + ".trace")) as f:
        want = f.read()
    assert r.stdout == want


@pytest.mark.parametrize("name", SCENARIOS)
def test_fault_sweep(driver, tiny_dir, name):
    r = _run(driver, tiny_dir, "--sweep", name)
    failures = [line for line in r.stderr.splitlines() if line.startswith("FAIL") or "Sanitizer" in line
                or "runtime error" in line]
    assert r.returncode == 0 and not failures, "\n".join(failures[:20]) + r.stderr[-3000:]
    assert f"sweep {name}:" in r.stdout and " 0 failures" in r.stdout
