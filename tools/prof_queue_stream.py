#!/usr/bin/env python3
"""The streaming work queue on the synthetic 1.7B model (measurement tool).

  python3 tools/prof_queue_stream.py [--reps 3] [--parent-lib PATH] [--out profiles/queue_stream_bench.txt]

Every figure is the median over --reps fresh processes (one child process per
repetition and quantity; the sides of a comparison alternate inside each
repetition).

  push   one multi-stream push of n streams x 4 frames, window full, host wall
         (ms, the median over 10 pushes): through qwen_tts_codec_mstream_push_any
         with the streams at mixed positions (72 + 5 s), against
         qwen_tts_codec_mstream_push with all streams at one position -- on the
         build --parent-lib names (the parent commit's) where given, else on
         this build
  queue  the 96-utterance EOS queue on 8 slots (bench.py --eos --queue 96
         --batch 8's utterances), chunk_frames 4: audio-s/s and slot occupancy
         of qwen_tts_generate_queue_stream beside qwen_tts_generate_queue, and
         every utterance's first-packet latency, from its admission (`next`)
         to its first chunk: median and p95; for contrast
         qwen_tts_generate_batch_stream on the first 8 utterances
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "qwen3-tts-c_amd"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
EOS_GAIN = 1.4      # bench.py --eos


def _model(eos=False):
    import qtts
    from synth_model import ensure_model
    base = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    if eos:         # the directory bench.py --eos uses
        md = ensure_model(os.path.join(base, f"1.7b_eos_gain{EOS_GAIN}"), "1.7b", overrides={"eos_gain": EOS_GAIN})
    else:
        md = ensure_model(os.path.join(base, "1.7b"), "1.7b")
    return qtts.QwenTTS(md)


def child_push(side, n, T=4):
    """{ms}: one push of n x T, window full; side mixed (push_any, positions 72 + 5 s) or equal (push)"""
    import numpy as np
    m = _model()
    rng = np.random.default_rng(n * 100 + T)
    warm, reps = 4, 10

    def codes(k, t):
        return rng.integers(0, 2048, size=(k, t, 16)).astype(np.int32)

    assert m.codec_mstream_begin(n, 4096) == 0
    assert m.codec_mstream_push(np.arange(n), codes(n, 72)) is not None      # fills the attention window
    if side == "mixed":
        for s in range(1, n):
            assert m.codec_mstream_push([s], codes(1, 5 * s)) is not None
        push = m.codec_mstream_push_any
    else:
        push = m.codec_mstream_push
    ts = []
    for _ in range(warm + reps):
        c = codes(n, T)
        t0 = time.perf_counter()
        o = push(np.arange(n), c)
        ts.append((time.perf_counter() - t0) * 1e3)
        assert o is not None
    m.close()
    return {"ms": statistics.median(ts[warm:])}


def child_queue(mode, nq=96, slots=8, chunk=4):
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model(eos=True)
    m.set_params(max_tokens=4096, fixed=0, seed=42, **DEFAULT)
    n = slots if mode == "batch_stream" else nq
    ids = [prompt_ids("p128", seed=1234 + i) for i in range(n)]
    spk, lang = ["aiden"] * n, ["english"] * n
    res = {}
    if mode == "queue":
        t0 = time.perf_counter()
        rc, audio = m.generate_queue(ids, spk, lang, slots=slots)
        wall = time.perf_counter() - t0
    elif mode == "queue_stream":
        seq, admitted, first = iter(range(n)), {}, {}

        def next_fn():
            u = next(seq, -1)
            admitted[u] = time.perf_counter()
            return u

        def on_chunk(u, a):
            if u not in first:
                first[u] = time.perf_counter()
        t0 = time.perf_counter()
        rc, audio = m.generate_queue_stream(ids, spk, lang, slots=slots, next_fn=next_fn, chunk_frames=chunk,
                                            on_chunk=on_chunk)
        wall = time.perf_counter() - t0
        # (the first `slots` admissions wait for the prompts' prefill; the refills are the steady state)
        lat = sorted((first[u] - admitted[u]) * 1e3 for u in first)
        refl = sorted((first[u] - admitted[u]) * 1e3 for u in first if u >= slots)
        res.update(fp_median_ms=statistics.median(lat), fp_p95_ms=lat[min(len(lat) - 1, int(0.95 * len(lat)))],
                   fp_refill_median_ms=statistics.median(refl) if refl else None,
                   fp_refill_p95_ms=refl[min(len(refl) - 1, int(0.95 * len(refl)))] if refl else None,
                   first_packet_ms=float(m.c.perf_first_packet_ms))
    else:
        t0 = time.perf_counter()
        rc, audio = m.generate_batch_stream(ids, spk, lang, chunk_frames=chunk)
        wall = time.perf_counter() - t0
        res.update(first_packet_ms=float(m.c.perf_first_packet_ms))
    assert rc == 0 and all(a is not None for a in audio)
    secs = sum(len(a) for a in audio) / 24000.0
    res.update(audio_s_per_s=secs / wall, total_ms=wall * 1e3, codec_ms=float(m.c.perf_codec_ms), audio_s=secs)
    if mode != "batch_stream":
        st = m.queue_stats()
        res.update(occupancy=st["occupancy"], frames=st["frames"], refills=st["refills"])
    else:
        fr = [len(a) // 1920 for a in audio]
        res.update(occupancy=sum(fr) / (len(fr) * (max(fr) + 1)), frames=max(fr))
    m.close()
    return res


def spawn(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["QTTS_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"child {args} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def med(rows, key):
    v = [r[key] for r in rows if r.get(key) is not None]
    return statistics.median(v) if v else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libqwen_tts_amd.so (the equal-position side)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_stream_bench.txt"))
    ap.add_argument("--skip-push", action="store_true")
    ap.add_argument("--skip-queue", action="store_true")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "push":
            print(json.dumps(child_push(a.child[1], int(a.child[2]))))
        else:
            print(json.dumps(child_queue(a.child[1])))
        return
    lines = [f"# tools/prof_queue_stream.py --reps {a.reps}: medians over {a.reps} fresh processes, synthetic 1.7B"]

    def say(s):
        lines.append(s)
        print(s, flush=True)
    if not a.skip_push:
        where = "the parent commit's build" if a.parent_lib else "this build"
        for n in (8, 32):
            rows = {"equal": [], "mixed": []}
            for _ in range(a.reps):
                rows["equal"].append(spawn(["push", "equal", n], a.parent_lib))
                rows["mixed"].append(spawn(["push", "mixed", n]))
            eq, mx = med(rows["equal"], "ms"), med(rows["mixed"], "ms")
            each = {k: " ".join(f"{r['ms']:.3f}" for r in v) for k, v in rows.items()}
            say(f"push n={n:2d} T=4 window full: equal positions, push on {where} {eq:7.3f} ms ({each['equal']})   "
                f"mixed positions, push_any {mx:7.3f} ms ({each['mixed']})   {100 * (mx / eq - 1):+.1f} %")
    if not a.skip_queue:
        plan = ["queue_stream", "queue", "batch_stream"]
        rows = {p: [] for p in plan}
        for _ in range(a.reps):
            for p in plan:
                rows[p].append(spawn(["queue", p]))
        for p in plan:
            r = rows[p]
            what = "first 8 utterances, lock step" if p == "batch_stream" else "96 EOS utterances on 8 slots"
            each = " ".join(f"{x['audio_s_per_s']:.1f}" for x in r)
            say(f"{p:12s} {what}, chunk 4: {med(r, 'audio_s_per_s'):7.1f} audio-s/s ({each})   occupancy {med(r, 'occupancy'):.4f}   "
                f"frames {med(r, 'frames'):.0f}   codec {med(r, 'codec_ms'):8.1f} ms of {med(r, 'total_ms'):8.1f} ms")
        r = rows["queue_stream"]
        say(f"queue_stream first packet per utterance, admission -> first chunk: median {med(r, 'fp_median_ms'):.2f} ms "
            f"p95 {med(r, 'fp_p95_ms'):.2f} ms over all 96; refilled utterances only: median "
            f"{med(r, 'fp_refill_median_ms'):.2f} ms p95 {med(r, 'fp_refill_p95_ms'):.2f} ms; call entry -> first "
            f"callback {med(r, 'first_packet_ms'):.2f} ms (batch_stream: {med(rows['batch_stream'], 'first_packet_ms'):.2f} ms)")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
