"""Incremental text input in the host orchestration (qwen_tts.c), on a CPU.

tests/host_trace/driver_text_feed.c runs scripted feeds against the unchanged
recording fake device tests/host_trace/fake_dev.c and the fake of the added
device entries, tests/host_trace/fake_textfeed.c, which keeps the gate's
arithmetic (rows published against frames drawn) and sits in front of four of
fake_dev.c's calls by the linker's --wrap.  It is built here with
AddressSanitizer and UBSan as a stand-alone executable.

Asserted on the recorded call order:
 - a frame is launched only when some live utterance has its row, and every
   row was appended before the frame that needs it (the fake's gate agrees with
   the host's count: a mismatch fails the call);
 - no frame is launched while every live utterance is starved, and before
   every wait = 1 callback everything decoded has been delivered;
 - frame 0 waits for every slot's row 0;
 - an utterance at its limit is retired;
 - a wait = 1 callback that pushes nothing fails the call ("feed made no
   progress"), an abort fails it, and a clean generate follows either;
 - the refusals come before the device is touched;
 - the fault sweep: with the K-th device call failing -- fake_dev.c's, then the
   text entries' -- the call fails, nothing stays armed, a clean generate
   follows, and the sanitizers stay silent.
The whole traces are pinned in tests/golden/host_trace_text_feed/ (a host
change that moves a device call on purpose records them again:
`driver_text_feed <tiny model dir> --trace NAME > NAME.trace` for every NAME).
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "qwen3-tts-c_amd", "csrc", "host")
SRC = os.path.join(HERE, "host_trace")
GOLD = os.path.join(HERE, "golden", "host_trace_text_feed")
NAMES = ["starve", "batch", "eos", "idle", "abort", "refusals"]
WRAPPED = ["qtts_dev_prompt", "qtts_dev_frame", "qtts_dev_poll", "qtts_dev_retire"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_trace_text_feed") / "driver_text_feed")
    srcs = [os.path.join(SRC, f) for f in ("driver_text_feed.c", "fake_textfeed.c", "fake_dev.c")]
    srcs += [os.path.join(HOST, f) for f in ("qwen_tts.c", "qjson.c", "wav.c", "bpe.c")]
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, *srcs, "-lm",
                    "-Wl," + ",".join("--wrap=" + w for w in WRAPPED)], check=True)
    return exe


@pytest.fixture(scope="module")
def traces(driver, tiny_dir):
    names = subprocess.run([driver, tiny_dir, "--list"], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert names == NAMES
    out = {}
    for name in names:
        r = subprocess.run([driver, tiny_dir, "--trace", name], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Sanitizer" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
        out[name] = r.stdout
    return out


@pytest.mark.parametrize("name", NAMES)
def test_trace_is_the_recorded_one(traces, name):
    with open(os.path.join(GOLD, name + ".trace")) as f:
        assert traces[name] == f.read()


def test_golden_directory_holds_exactly_the_scenarios():
    assert sorted(os.listdir(GOLD)) == sorted(n + ".trace" for n in NAMES)


def replay(trace, nb):
    """Walks one fed run's trace with the row rule: rows / open per slot from the
    text_open / text_append lines, frames per slot from the frame lines.  Returns
    the events [(kind, data)] it checked: ("frame", ran), ("wait", None), ("held", [slots])."""
    rows, opened, frames, retired = [0] * nb, [False] * nb, [0] * nb, [False] * nb
    delivered, events, limit = [0] * nb, [], None
    lines = trace.splitlines()
    for i, l in enumerate(lines):
        m = re.match(r"begin nb=\d+ max_frames=(\d+)", l)
        if m:
            limit = int(m.group(1))
        m = re.match(r"text_open b=(\d+)", l)
        if m:
            opened[int(m.group(1))] = True
        m = re.match(r"text_append b=(\d+) n=(\d+) close=(\d) .* rows=(\d+)", l)
        if m:
            b, n, c = int(m.group(1)), int(m.group(2)), int(m.group(3))
            assert opened[b], l                               # never after the close
            rows[b] += n + c
            assert rows[b] == int(m.group(4))
            if c:
                opened[b] = False
        m = re.match(r"retire b=(\d+)", l)
        if m:
            b = int(m.group(1))
            assert frames[b] == limit, (l, frames)            # retired at the limit, not before
            retired[b] = True
        m = re.match(r"audio u=(\d+) samples=(\d+)", l)
        if m:
            assert int(m.group(2)) % 1920 == 0 and int(m.group(2)) > 0
            delivered[int(m.group(1))] += int(m.group(2)) // 1920
        m = re.match(r"feed wait=(\d)((?: u\d+=\d+/\d+/\d)+)", l)
        if m:
            st = [tuple(int(x) for x in s.split("=")[1].split("/")) for s in m.group(2).split()]
            if m.group(1) == "1" and limit is not None:
                # flush before wait = 1: what the host counts as decoded is delivered
                # (an utterance that drew EOS has one frame fewer than the host launched for it)
                for b in range(nb):
                    assert delivered[b] in (st[b][1], st[b][1] - 1), (l, delivered)
                events.append(("wait", None))
        m = re.match(r"frame step=(\d+)", l)
        if m and limit is not None:
            step = int(m.group(1))
            held = []
            if i + 1 < len(lines) and lines[i + 1].startswith("gate held=["):
                held = [int(x) for x in lines[i + 1][len("gate held=["):-1].split(",")]
            starved = [b for b in range(nb) if opened[b] and frames[b] >= rows[b] and not retired[b]
                       and frames[b] < limit]
            # the fake's gate (what the device would hold) is the row rule applied to what was appended
            # BEFORE this launch; an EOS-stopped slot is not in either list
            assert set(held) <= set(starved), (l, held, starved)
            if step == 0:
                assert not starved, (l, starved)              # frame 0 waits for every slot's row 0
            ran = [b for b in range(nb) if b not in starved and not retired[b] and frames[b] < limit]
            assert ran, (l, "a frame launched with every live slot starved")
            for b in ran:
                frames[b] += 1
            events.append(("frame", ran))
            if held:
                events.append(("held", held))
    return events, frames, delivered


def fed_part(trace):
    """the first fed call of a trace: up to its result line"""
    return trace[:trace.index("\nfed ") + 1]


def test_starve_appends_before_frames_and_flushes_before_wait(traces):
    t = traces["starve"]
    events, frames, delivered = replay(fed_part(t), 1)
    assert frames == [8] and delivered == [8]
    assert [k for k, _ in events].count("wait") == 3          # after the start: three starvations
    assert "retire b=0" in t and "fed starve -> 0" in t
    # the prompt holds the first content id alone: the tts_eos row is its only trailing row
    assert re.search(r"prompt b=0 text_ids=\[151644,77091,198,151671,151672,151673,2354\] .* n_trailing=1 ", t)
    # no frame between a starved wait = 0 callback and the wait = 1 that follows it
    assert not re.search(r"feed wait=0 u0=\d+/\d+/1\n(?:poll.*\n|codec.*\n|audio.*\n)*frame", t)


def test_batch_holds_one_slot(traces):
    t = traces["batch"]
    events, frames, delivered = replay(fed_part(t), 3)
    assert frames == [6, 6, 6] and delivered == [6, 6, 6]
    held = [d for k, d in events if k == "held"]
    assert held == [[1]] * 3 and "held 1=3" in t              # slot 1 sat out three launched frames
    assert all(f"retire b={b}" in t for b in range(3))
    assert "wait=1" not in t.split("\nprefill\n")[1]              # some slot could always advance
    assert "fed batch -> 0" in t


def test_eos_mode(traces):
    t = traces["eos"]
    assert "fed eos -> 0" in t
    part = t.split("\nprefill\n")[1]
    # utterance 1 starves at its eos row while utterance 0 runs to its EOS; then the wait = 1
    assert part.count("gate held=[1]") >= 3 and part.count("feed wait=1") == 1
    assert " feed_close u=1 -> 0\n feed_ids u=0 n=1 -> 0" in t   # the push to a stopped utterance: 0
    assert t.count("text_append b=0") == 1                     # ... and nothing reached the device
    assert "retire" not in t                                   # both drew EOS before the limit


def test_no_progress_and_abort(traces):
    for name, msg in (("idle", "feed made no progress"), ("abort", "the feed callback aborted the call (-7)")):
        t = traces[name]
        assert msg in t and f"fed {name} -> -1" in t
        head, tail = t.split(f"fed {name} -> -1")
        assert "out 0 samples=0" in tail and "generate (after) -> audio" in tail
        assert "frame" not in head[head.index(msg):]           # the loop ends there
    assert traces["idle"].split("generate (after)")[1] == traces["abort"].split("generate (after)")[1]


def test_refusals_come_before_the_device(traces):
    t = traces["refusals"]
    before = t[:t.index("fed 65 -> -1")]
    assert not re.search(r"^(begin|prompt|prefill|frame|text_open|text_append)\b", before, re.M)
    for call in ("fed empty", "fed forced", "fed no callback", "fed 65"):
        assert f"{call} -> -1" in t
    assert t.count("armed after: force=0 sampling=0 instruct=0") == 5
    assert "generate (after) -> audio" in t


@pytest.mark.parametrize("name", NAMES)
def test_fault_sweep(driver, tiny_dir, name):
    r = subprocess.run([driver, tiny_dir, "--sweep", name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    failures = [line for line in r.stderr.splitlines() if line.startswith("FAIL") or "Sanitizer" in line
                or "runtime error" in line]
    assert r.returncode == 0 and not failures, "\n".join(failures[:20]) + r.stderr[-3000:]
    assert f"sweep {name}:" in r.stdout and " 0 failures" in r.stdout
