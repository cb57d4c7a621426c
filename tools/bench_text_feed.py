#!/usr/bin/env python3
"""Incremental text input on the synthetic 1.7B model (measurement tool).

  python3 tools/bench_text_feed.py [--reps 3] [--out profiles/text_feed_bench.txt]

Every figure is the median over --reps fresh processes (one child process per
repetition and quantity; the two sides of a comparison alternate inside each
repetition).

  first    first packet (ms) of qwen_tts_generate_fed_stream fed two ids at the
           start and the rest at the next callback, beside
           qwen_tts_generate_stream on the whole template (p128 prompt, 16 frames)
  append   one qwen_tts_feed_ids of 1 id and of 16 ids inside a wait = 0
           callback of a running decode: the call's host wall (us; no sync in
           it), and the wall of the same call followed by a wait for the
           context stream with nothing else queued (us: launches + kernels);
           the device time of one qtts_dev_text_append of the same size, from
           events on the context stream (qtts_dev_text_append_ms)
  speed    all text at the first callback against qwen_tts_generate_batch_stream,
           batch 1 and 8, 128 frames, chunk 4: audio-s/s and the ratio
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "qwen3-tts-c_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]


def _model():
    import qtts
    from synth_model import ensure_model
    md = ensure_model(os.path.join(os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models"), "1.7b"), "1.7b")
    return qtts.QwenTTS(md)


def _feed_all(contents):
    sent = [False] * len(contents)

    def feed(h, wait):
        for u, ids in enumerate(contents):
            if not sent[u]:
                assert h.push(u, ids) == 0 and h.close(u) == 0
                sent[u] = True
    return feed


def child_first(mode):
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model()
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    tpl = prompt_ids("p128", seed=1234)
    ids = tpl[3:-5]
    res = None
    for _ in range(2):   # (one warm-up call)
        if mode == "fed":
            st = dict(n=0)

            def feed(h, wait):
                st["n"] += 1
                if st["n"] == 1:
                    assert h.push(0, ids[:2]) == 0
                elif st["n"] == 2:
                    assert h.push(0, ids[2:]) == 0 and h.close(0) == 0
            a = m.generate_fed_stream(feed, "aiden", "english", chunk_frames=4)
        else:
            a = m.generate_stream(tpl, "aiden", "english", chunk_frames=4)
        assert a is not None
        res = {"first_packet_ms": float(m.c.perf_first_packet_ms)}
    m.close()
    return res


def child_append(n):
    import numpy as np
    import qtts
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model()
    lib = qtts.lib()
    m.set_params(max_tokens=4096, fixed=64, seed=42, **DEFAULT)
    ids = prompt_ids("p128", seed=1234)[3:-5]
    grp = np.ascontiguousarray((ids * 2)[:n], np.int32)
    host, synced = [], []
    st = dict(n=0)

    def feed(h, wait):
        st["n"] += 1
        if st["n"] == 1:
            assert h.push(0, ids) == 0
            return
        if st.get("closed"):
            return
        if h.state(0)[1] >= 60:
            h.close(0)
            st["closed"] = True
            return
        p = grp.ctypes.data_as(C.POINTER(C.c_int))
        if st["n"] % 2 == 0:
            t0 = time.perf_counter()
            rc = lib.qwen_tts_feed_ids(h._p, 0, p, n)
            host.append((time.perf_counter() - t0) * 1e6)
        else:
            lib.qtts_hip_sync()                      # nothing queued in front of it
            t0 = time.perf_counter()
            rc = lib.qwen_tts_feed_ids(h._p, 0, p, n)
            lib.qtts_hip_sync()
            synced.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0
    a = m.generate_fed_stream(feed, "aiden", "english", chunk_frames=4)
    assert a is not None
    m.close()
    return {"host_us": statistics.median(host[3:]), "synced_us": statistics.median(synced[3:])}


class GenParams(C.Structure):   # qtts_gen_params_t
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("top_k", C.c_int), ("st_temperature", C.c_float), ("st_top_p", C.c_float), ("st_top_k", C.c_int),
                ("fixed_codec_tokens", C.c_int), ("seed", C.c_int)]


def child_append_dev(n):
    """device time of one append of n ids, from events (qtts_dev_text_append_ms), on an idle stream"""
    import numpy as np
    import qtts
    from synth_model import prompt_ids
    m = _model()
    lib, dev = qtts.lib(), C.c_void_p(m.c.hip)
    ids = prompt_ids("p128", seed=1234)[3:-5]
    gp = GenParams(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 4, 42)
    assert lib.qtts_dev_begin(dev, 1, 4, 16, C.byref(gp)) == 0
    text, plan = [151671, 151673, ids[0]], [2, -1, 0, 0, 0, 1, -1, 1, 0, 0]   # (the one-row prompt of the kernel test)
    assert lib.qtts_dev_prompt(dev, 0, (C.c_int * 3)(*text), 3, (C.c_int * 10)(*plan), 2, 1, 1, 0) == 0
    assert lib.qtts_dev_text_open(dev, 0) == 0
    assert lib.qtts_dev_reserve(dev, 2048) == 0                               # (no growth inside the timed appends)
    grp = np.ascontiguousarray((ids * 2)[:n], np.int32)
    ms, out = C.c_float(0), []
    for _ in range(40):
        assert lib.qtts_dev_text_append_ms(dev, 0, grp.ctypes.data_as(C.POINTER(C.c_int)), n, 0, C.byref(ms)) == 0
        out.append(ms.value * 1e3)
    m.close()
    return {"dev_us": statistics.median(out[5:])}


def child_speed(mode, batch, frames=128, chunk=4):
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model()
    m.set_params(max_tokens=4096, fixed=frames, seed=42, **DEFAULT)
    tpl = [prompt_ids("p128", seed=1234 + b) for b in range(batch)]
    res = None
    for _ in range(2):
        t0 = time.perf_counter()
        if mode == "fed":
            rc, audio = m.generate_fed_batch_stream(batch, _feed_all([t[3:-5] for t in tpl]), ["aiden"] * batch,
                                                    ["english"] * batch, chunk_frames=chunk)
        else:
            rc, audio = m.generate_batch_stream(tpl, ["aiden"] * batch, ["english"] * batch, chunk_frames=chunk)
        wall = time.perf_counter() - t0
        assert rc == 0 and all(a is not None for a in audio)
        res = {"audio_s_per_s": sum(len(a) for a in audio) / 24000.0 / wall, "total_ms": wall * 1e3,
               "talker_ms": float(m.c.perf_talker_ms), "codec_ms": float(m.c.perf_codec_ms)}
    m.close()
    return res


def spawn(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def med(rows, key):
    return statistics.median(r[key] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_feed_bench.txt"))
    a = ap.parse_args()
    if a.child:
        kind = a.child[0]
        if kind == "first":
            print(json.dumps(child_first(a.child[1])))
        elif kind == "append":
            print(json.dumps(child_append(int(a.child[1]))))
        elif kind == "append_dev":
            print(json.dumps(child_append_dev(int(a.child[1]))))
        else:
            print(json.dumps(child_speed(a.child[1], int(a.child[2]))))
        return
    lines = [f"# tools/bench_text_feed.py --reps {a.reps}: medians over {a.reps} fresh processes, synthetic 1.7B"]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    rows = {"fed": [], "stream": []}
    for _ in range(a.reps):
        for k in rows:
            rows[k].append(spawn("first", k))
    say(f"first packet, p128 prompt: fed (2 ids, then the rest) {med(rows['fed'], 'first_packet_ms'):6.2f} ms   "
        f"generate_stream {med(rows['stream'], 'first_packet_ms'):6.2f} ms")
    for n in (1, 16):
        r = [spawn("append", n) for _ in range(a.reps)]
        d = [spawn("append_dev", n) for _ in range(a.reps)]
        say(f"append of {n:2d} id(s): qwen_tts_feed_ids host wall {med(r, 'host_us'):7.1f} us   "
            f"call + wait for the idle stream {med(r, 'synced_us'):7.1f} us   device time from events "
            f"{med(d, 'dev_us'):7.1f} us")
    for batch in (1, 8):
        rows = {"fed": [], "unfed": []}
        for _ in range(a.reps):
            for k in rows:
                rows[k].append(spawn("speed", k, batch))
        f, u = med(rows["fed"], "audio_s_per_s"), med(rows["unfed"], "audio_s_per_s")
        say(f"full speed batch {batch}, 128 frames chunk 4: fed {f:7.1f} audio-s/s   generate_batch_stream {u:7.1f} "
            f"audio-s/s   ratio {f / u:5.3f}   (talker ms {med(rows['fed'], 'talker_ms'):.1f} vs "
            f"{med(rows['unfed'], 'talker_ms'):.1f}, codec ms {med(rows['fed'], 'codec_ms'):.1f} vs "
            f"{med(rows['unfed'], 'codec_ms'):.1f})")
    with open(a.out, "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
