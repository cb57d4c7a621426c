"""The instruct arming in the host orchestration (qwen_tts.c), on a CPU.

tests/host_trace/driver_instruct.c runs the instruct scenarios against the
unchanged recording fake device tests/host_trace/fake_dev.c; it is built here
with AddressSanitizer and UBSan as a stand-alone executable.

The fake logs every qtts_dev_prompt: p_len, n_trailing and pad_row in full, the
text ids and the plan as length + FNV-1a.  The expected ids and plan are laid
out by tests/instruct_layout.py from the layout's description (first checked
against the unarmed twin of each scenario) and hashed the same way:

 - p_len = the unarmed p_len + ni, n_trailing and pad_row unchanged;
 - the ni instruct ids stand behind the utterance's own text rows, and the
   first ni plan rows are {that text row, -1, 2, b, i}, the others shifted;
 - a NULL or empty entry's line equals the unarmed one;
 - the queue indexes the arming by input order, whatever the slot;
 - a count mismatch and every voice-clone entry return -1 before the device is
   touched, disarm, and a clean call follows;
 - the fault sweep: with the K-th device call failing all three armings are
   consumed, a clean generate follows, and the sanitizers stay silent.
"""
import json
import os
import re
import struct
import subprocess

import pytest

from instruct_layout import layout

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qwen3-tts-c_amd", "csrc", "host")
SRC = os.path.join(HERE, "host_trace")

HEAD, TAIL = [151644, 77091, 198], [151645, 198, 151644, 77091, 198]
TEXTS = [HEAD + body + TAIL for body in (
    [2354, 2244, 2355, 4041], [1111, 2222, 3333, 4444, 5555, 6666], [901, 902, 903],
    [7001, 7002, 7003, 7004, 7005, 7006, 7007, 7008], [314, 159, 265, 358, 979],
    [27, 18, 28, 18, 28, 45, 90, 45, 23, 53], [4242, 4243])]
SPK = ["aiden", "aiden", None, "aiden", "aiden", "aiden", None]
LANG = ["english", None, "english", "auto", "english", "english", "english"]
INS_A = [151644, 872, 198, 501, 502, 503, 151645, 198]
INS_B = [151644, 872, 198] + list(range(61, 76)) + [151645, 198]
INS_ONE = [777]
INS7 = [INS_A, [], INS_B, INS_A, [], INS_ONE, INS_B]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_trace_instruct") / "driver_instruct")
    srcs = [os.path.join(SRC, "driver_instruct.c"), os.path.join(SRC, "fake_dev.c")]
    srcs += [os.path.join(HOST, f) for f in ("qwen_tts.c", "qjson.c", "wav.c", "bpe.c")]
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, *srcs, "-lm"], check=True)
    return exe


@pytest.fixture(scope="module")
def traces(driver, tiny_dir):
    out = {}
    names = subprocess.run([driver, tiny_dir, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for name in names:
        r = subprocess.run([driver, tiny_dir, "--trace", name], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
        out[name] = r.stdout
    return out


def fnv(ints):
    h = 2166136261
    for b in struct.pack(f"<{len(ints)}i", *ints):
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def arr(key, ints):
    """the fake's rendering of an int array (fake_dev.c lg_ia)"""
    if len(ints) > 8:
        return f" {key}=len {len(ints)} fnv {fnv(ints):08x}"
    return f" {key}=[" + ",".join(str(i) for i in ints) + "]"


def prompt_line(cfg, u, ins, b):
    text, plan, p_len, nt = layout(cfg, TEXTS[u], SPK[u], LANG[u], ins, b)
    flat = [v for row in plan for v in row]
    return f"prompt b={b}" + arr("text_ids", text) + arr("plan", flat) + f" p_len={p_len} n_trailing={nt} pad_row=3"


def prompts(trace):
    return [l for l in trace.splitlines() if l.startswith("prompt b=")]


def fields(line):
    m = re.search(r"p_len=(\d+) n_trailing=(\d+) pad_row=(-?\d+)", line)
    return tuple(int(g) for g in m.groups())


@pytest.fixture(scope="module")
def cfg(tiny_dir):
    with open(os.path.join(tiny_dir, "config.json")) as f:
        return json.load(f)


def test_layout_here_reproduces_the_unarmed_prompts(traces, cfg):
    """the check of the checker: with no instruct, layout() gives the lines the host logs today"""
    assert prompts(traces["single_plain"]) == [prompt_line(cfg, 0, [], 0)] * 2
    assert prompts(traces["batch_plain"]) == [prompt_line(cfg, u, [], u) for u in range(3)]
    got = prompts(traces["queue_plain"])
    assert len(got) == 7 and sorted(got[:3]) == sorted(prompt_line(cfg, u, [], u) for u in range(3))


def test_single(traces, cfg):
    t = traces["single"]
    assert "set_utterance_instruct -> 0" in t
    armed, after = prompts(t)
    plain = prompts(traces["single_plain"])[0]
    assert armed == prompt_line(cfg, 0, INS_A, 0)
    p, ntr, pad = fields(plain)
    assert fields(armed) == (p + len(INS_A), ntr, pad)
    assert after == plain                                   # one-shot: the call after an armed call is plain
    assert t.count("generate -> audio") == 1 and "generate_stream (after) -> audio" in t
    assert "instruct=1" not in t                            # consumed by the call that used it
    # (the forced codes armed beside it were applied: both armings serve one call)
    assert "force_codes -> 0" in t and re.search(r"^force ", t, re.M)


def test_batch_with_a_null_entry(traces, cfg):
    t = traces["batch"]
    got, plain = prompts(t), prompts(traces["batch_plain"])
    ins = [INS_B, [], INS_ONE]
    assert got == [prompt_line(cfg, u, ins[u], u) for u in range(3)]
    assert got[1] == plain[1]                               # a NULL entry's line equals the unarmed one
    for u in range(3):
        p, ntr, pad = fields(plain[u])
        assert fields(got[u]) == (p + len(ins[u]), ntr, pad)
    m = re.search(r"begin nb=3 max_frames=\d+ max_prefill=(\d+)", t)
    assert int(m.group(1)) == max(fields(l)[0] for l in got)   # the state is sized for the longest prompt
    assert "generate_batch_stream -> 0" in t and t.count("slot_params") == 3   # sampling served beside it


def test_queue_with_refills(traces, cfg):
    t = traces["queue"]
    assert "generate_queue -> 0" in t
    got = prompts(t)
    assert len(got) == 7 and t.count("\nrefill b=") == 4
    # admission is in input order here: utterance u's prompt is the u-th, on whatever slot
    for u, line in enumerate(got):
        b = int(re.match(r"prompt b=(\d+)", line).group(1))
        assert 0 <= b < 3
        assert line == prompt_line(cfg, u, INS7[u], b), u
    # NULL and "" entries: the unarmed utterance's line, but for the slot it landed in (the fake's EOS
    # frames follow the text-id hash, so the armed run admits on other slots than the unarmed one)
    plain = prompts(traces["queue_plain"])
    slot = lambda l: int(re.match(r"prompt b=(\d+)", l).group(1))
    for u in (1, 4):
        assert plain[u] == prompt_line(cfg, u, [], slot(plain[u])) and got[u] == prompt_line(cfg, u, [], slot(got[u]))
        assert fields(got[u]) == fields(plain[u])
    assert {int(re.match(r"prompt b=(\d+)", l).group(1)) for l in got[3:]} <= {0, 1, 2}
    m = re.search(r"begin nb=3 max_frames=\d+ max_prefill=(\d+)", t)
    assert int(m.group(1)) == max(fields(l)[0] for l in got)


def test_count_mismatch_disarms_before_the_device(traces, cfg):
    t = traces["count"]
    head, tail = t.split("generate (after)")[0], t
    assert "generate_batch (2 instructs) -> -1" in head and "generate_queue_stream (2 instructs) -> -1" in head
    # nothing reached the device before the clean call
    before = head[:head.index("generate_queue_stream (2 instructs) -> -1")]
    assert not re.search(r"^(begin|prompt|prefill|frame)\b", before, re.M)
    assert head.count("armed after: force=0 sampling=0 instruct=0") == 2
    assert prompts(tail) == [prompt_line(cfg, 0, [], 0)] and "generate (after) -> audio" in tail


def test_voice_clone_refuses(traces, cfg):
    t = traces["clone"]
    for call in ("generate_voice_clone", "generate_voice_clone_stream", "generate_voice_clone_audio",
                 "generate_voice_clone_audio_stream"):
        assert f"{call} -> NULL" in t, call
    assert "generate_voice_queue -> -1" in t and "generate_voice_queue_stream -> -1" in t
    assert t.count("armed after: force=0 sampling=0 instruct=0") == 7
    before = t[:t.index("generate_voice_queue_stream -> -1")]
    assert not re.search(r"^(begin|prompt|prompt_ref|prefill|frame|speaker_embed|encode_audio)\b", before, re.M)
    assert prompts(t) == [prompt_line(cfg, 0, [], 0)] and "generate (after) -> audio" in t


@pytest.mark.parametrize("name", ["single", "batch", "queue", "count", "clone"])
def test_fault_sweep(driver, tiny_dir, name):
    r = subprocess.run([driver, tiny_dir, "--sweep", name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    failures = [line for line in r.stderr.splitlines() if line.startswith("FAIL") or "Sanitizer" in line
                or "runtime error" in line]
    assert r.returncode == 0 and not failures, "\n".join(failures[:20]) + r.stderr[-3000:]
    assert f"sweep {name}:" in r.stdout and " 0 failures" in r.stdout
