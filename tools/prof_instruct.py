#!/usr/bin/env python3
"""Instruct prompts and the instruct prefix cache on the synthetic 1.7B model
(measurement tool).

  python3 tools/prof_instruct.py [--reps 3] [--parent-lib PATH] [--out profiles/instruct_bench.txt]

Every figure is the median over --reps fresh processes (one child process per
repetition and quantity; the sides of a comparison alternate inside each
repetition).

  stream   qwen_tts_generate_stream of one utterance (bench.py's P128 prompt,
           16 frames, chunk 4): the first packet and the talker prefill (ms),
           unarmed, and with an instruct of 16 and of 80 ids in three
           conditions each: cache off (the instruct rows are ordinary rows of
           the one prefill pass), miss (the prefix pass, a save, the rest) and
           hit (a restore, the rest).  Each child warms up on ANOTHER instruct
           of the same length, so the measured call runs warm kernels and, for
           `miss`, still finds no entry; `hit` repeats the measured instruct.
  queue    96 EOS utterances (bench.py --eos --queue 96's prompts) on 8 slots,
           chunk_frames 4, all with one 80-id instruct, through
           qwen_tts_generate_queue_stream: audio-s/s and every utterance's first
           packet from its admission (`next`) to its first chunk (median, p95),
           cache on against cache off
  bench    bench.py --gpus 1 --steps 3 --warmup 1 [--batch 8] on this build and
           on the parent's (the unchanged paths)
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


def _instruct(n, seed):
    import numpy as np
    return np.random.default_rng(seed).integers(1000, 100000, size=n).tolist()


def child_stream(cond, n):
    """{first_packet_ms, prefill_ms, rows}: cond in unarmed / off / miss / hit, n instruct ids"""
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model()
    m.set_params(max_tokens=4096, fixed=16, seed=42, **DEFAULT)
    ids = prompt_ids("p128", seed=1234)
    m.prefix_cache(0 if cond in ("unarmed", "off") else 16)

    def call(instruct):
        if instruct is not None:
            m.set_utterance_instruct([instruct])
        r0 = m.prefix_counters()
        assert m.generate_stream(ids, "aiden", "english", chunk_frames=4) is not None
        r1 = m.prefix_counters()
        return {"first_packet_ms": float(m.c.perf_first_packet_ms), "prefill_ms": float(m.c.perf_prefill_ms),
                "rows": r1[2] - r0[2], "hits": r1[0] - r0[0], "misses": r1[1] - r0[1]}

    measured = None if cond == "unarmed" else _instruct(n, 1)
    for _ in range(2):      # warm: the same row counts and kernels on another instruct
        call(None if cond == "unarmed" else _instruct(n, 2))
    if cond == "hit":
        call(measured)
    res = call(measured)
    res["entry_bytes"] = m.prefix_cache_bytes()
    m.close()
    return res


def child_queue(cache, nq=96, slots=8, chunk=4, n=80):
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model(eos=True)
    m.set_params(max_tokens=4096, fixed=0, seed=42, **DEFAULT)
    m.prefix_cache(16 if cache == "on" else 0)
    ids = [prompt_ids("p128", seed=1234 + i) for i in range(nq)]
    instruct = _instruct(n, 1)
    res = {}
    for call in ("first", "second"):
        seq, admitted, first = iter(range(nq)), {}, {}

        def next_fn():
            u = next(seq, -1)
            admitted[u] = time.perf_counter()
            return u

        def on_chunk(u, a):
            if u not in first:
                first[u] = time.perf_counter()
        c0 = m.prefix_counters()
        m.set_utterance_instruct([instruct] * nq)
        t0 = time.perf_counter()
        rc, audio = m.generate_queue_stream(ids, ["aiden"] * nq, ["english"] * nq, slots=slots, next_fn=next_fn,
                                            chunk_frames=chunk, on_chunk=on_chunk)
        wall = time.perf_counter() - t0
        assert rc == 0 and all(a is not None for a in audio)
        c1 = m.prefix_counters()
        secs = sum(len(a) for a in audio) / 24000.0
        st = m.queue_stats()
        lat = sorted((first[u] - admitted[u]) * 1e3 for u in first)
        refl = sorted((first[u] - admitted[u]) * 1e3 for u in first if u >= slots)
        res[call] = {"audio_s_per_s": secs / wall, "total_ms": wall * 1e3, "audio_s": secs, "occupancy": st["occupancy"],
                     "frames": st["frames"], "refills": st["refills"], "rows": c1[2] - c0[2], "hits": c1[0] - c0[0],
                     "misses": c1[1] - c0[1], "prefill_ms": float(m.c.perf_prefill_ms),
                     "fp_median_ms": statistics.median(lat), "fp_p95_ms": lat[min(len(lat) - 1, int(0.95 * len(lat)))],
                     "fp_refill_median_ms": statistics.median(refl),
                     "fp_refill_p95_ms": refl[min(len(refl) - 1, int(0.95 * len(refl)))],
                     "first_packet_ms": float(m.c.perf_first_packet_ms)}
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
    print(f"  done: {' '.join(str(x) for x in args)}", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def bench(extra, lib=None):
    env = dict(os.environ)
    if lib:
        env["QTTS_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"]
                       + extra, capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py {extra} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    for line in reversed(r.stdout.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError("bench.py printed no result line")


def med(rows, key):
    v = [r[key] for r in rows if r.get(key) is not None]
    return statistics.median(v) if v else float("nan")


def each(rows, key, fmt="{:.3f}"):
    return " ".join(fmt.format(r[key]) for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libqwen_tts_amd.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instruct_bench.txt"))
    ap.add_argument("--only", default="stream,queue,bench", help="comma list of stream, queue, bench")
    ap.add_argument("--append", action="store_true", help="append to --out instead of rewriting it")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "stream":
            print(json.dumps(child_stream(a.child[1], int(a.child[2]))))
        else:
            print(json.dumps(child_queue(a.child[1])))
        return
    only = a.only.split(",")
    where = "the parent commit's build" if a.parent_lib else "this build"
    with open(a.out, "a" if a.append else "w") as f:
        f.write(f"# tools/prof_instruct.py --reps {a.reps} --only {a.only}: medians over {a.reps} fresh processes, "
                "synthetic 1.7B\n")

    def say(s):     # (written as it goes: a run cut short keeps what it measured)
        print(s, flush=True)
        with open(a.out, "a") as f:
            f.write(s + "\n")
    if "stream" in only:
        plan = [("unarmed", 0)] + [(c, n) for n in (16, 80) for c in ("off", "miss", "hit")]
        rows = {p: [] for p in plan}
        for _ in range(a.reps):
            for p in plan:
                rows[p].append(spawn(["stream", p[0], p[1]]))
        for p in plan:
            r = rows[p]
            say(f"stream {p[0]:7s} instruct {p[1]:2d} ids: first packet {med(r, 'first_packet_ms'):7.2f} ms "
                f"({each(r, 'first_packet_ms', '{:.2f}')})   prefill {med(r, 'prefill_ms'):6.2f} ms "
                f"({each(r, 'prefill_ms', '{:.2f}')})   {int(med(r, 'rows'))} rows prefilled, "
                f"{int(med(r, 'hits'))} hit {int(med(r, 'misses'))} miss, cache {med(r, 'entry_bytes') / 1e6:.2f} MB")
    if "queue" in only:
        rows = {"on": [], "off": []}
        for _ in range(a.reps):
            for c in ("on", "off"):
                rows[c].append(spawn(["queue", c]))
        for c in ("on", "off"):
            for call in ("first", "second"):
                r = [x[call] for x in rows[c]]
                say(f"queue_stream cache {c:3s} {call:6s} call, 96 EOS utterances with one 80-id instruct on 8 slots, chunk 4: "
                    f"{med(r, 'audio_s_per_s'):7.1f} audio-s/s ({each(r, 'audio_s_per_s', '{:.1f}')})   occupancy "
                    f"{med(r, 'occupancy'):.3f}   {int(med(r, 'frames'))} frames, {int(med(r, 'refills'))} refills, "
                    f"{med(r, 'audio_s'):.1f} s audio in {med(r, 'total_ms'):7.1f} ms   {int(med(r, 'rows'))} rows prefilled, "
                    f"{int(med(r, 'hits'))} hits {int(med(r, 'misses'))} misses   first packet per utterance: median "
                    f"{med(r, 'fp_median_ms'):6.2f} ms p95 {med(r, 'fp_p95_ms'):6.2f} ms, refilled only: median "
                    f"{med(r, 'fp_refill_median_ms'):6.2f} ms ({each(r, 'fp_refill_median_ms', '{:.2f}')}) p95 "
                    f"{med(r, 'fp_refill_p95_ms'):6.2f} ms; the call's first packet {med(r, 'first_packet_ms'):7.2f} ms "
                    f"({each(r, 'first_packet_ms', '{:.2f}')}), initial prefill {med(r, 'prefill_ms'):6.2f} ms")
    if "bench" in only:
        for extra in ([], ["--batch", "8"]):
            rows = {"parent": [], "this": []}
            for _ in range(a.reps):
                rows["parent"].append(bench(extra, a.parent_lib))
                rows["this"].append(bench(extra))
            key = "value" if "value" in rows["this"][0] else "audio_s_per_s"
            p, t = med(rows["parent"], key), med(rows["this"], key)
            say(f"bench.py --gpus 1 --steps 3 --warmup 1 {' '.join(extra):9s}: {where} {p:7.2f} ({each(rows['parent'], key, '{:.2f}')})"
                f"   this build {t:7.2f} ({each(rows['this'], key, '{:.2f}')}) audio-s/s   {100 * (t / p - 1):+.1f} %")


if __name__ == "__main__":
    main()
