#!/usr/bin/env python3
"""The ragged multi-stream push and the streamed voice-clone batch on the
synthetic 1.7B model (measurement tool).

  python3 tools/prof_vc_batch_stream.py [--reps 3] [--parent-lib PATH] [--out profiles/vc_batch_stream_bench.txt]

Every figure is the median over --reps fresh processes (one child process per
repetition and quantity; the sides of a comparison alternate inside each
repetition).

  prime  n streams (8, 32) from position 0, reference lengths spread evenly
         over 40..80 frames, host wall of the whole priming (ms, the median
         over 5 primings, each after a begin):
           ragged    one qwen_tts_codec_mstream_push_ragged
           separate  one qwen_tts_codec_mstream_push_any per stream, on the
                     build --parent-lib names (the parent commit's; the only
                     way it can prime ragged lengths), else on this build
           uniform   one push_any of all n streams at the largest length (80):
                     what the ragged push would cost if nothing were padding
  push   one push of n x 4 frames, window full, streams at 72 + 5 s, through
         push_any on this build and on the parent's (equal counts must not
         have become slower)
  vc     generate_voice_clone_batch_stream at batch 8, 63-frame references,
         128 frames, chunk_frames 4 (bench.py --voice-clone --vc-codes'
         inputs): first packet and audio-s/s, beside generate_voice_clone_batch
         on the same inputs and generate_voice_clone_stream at batch 1
  bench  bench.py --gpus 1 --steps 3 --warmup 1 [--batch 8] on this build and
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


def _model():
    import qtts
    from synth_model import ensure_model
    base = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    return qtts.QwenTTS(ensure_model(os.path.join(base, "1.7b"), "1.7b"))


def ref_lengths(n):
    return [40 + (40 * s) // max(n - 1, 1) for s in range(n)]


def child_prime(side, n):
    """{ms}: priming n streams with 40..80 reference frames from position 0"""
    import numpy as np
    m = _model()
    rng = np.random.default_rng(n)
    lens = ref_lengths(n)
    codes = [rng.integers(0, 2048, size=(80, 16)).astype(np.int32) for _ in range(n)]
    warm, reps = 2, 5
    ts = []
    for _ in range(warm + reps):
        assert m.codec_mstream_begin(n, 256) == 0
        t0 = time.perf_counter()
        if side == "ragged":
            o = m.codec_mstream_push_ragged(np.arange(n), [c[:k] for c, k in zip(codes, lens)])
            assert o is not None
        elif side == "separate":
            for s in range(n):
                assert m.codec_mstream_push_any([s], codes[s][None, :lens[s]]) is not None
        else:
            assert m.codec_mstream_push_any(np.arange(n), np.stack(codes)) is not None
        ts.append((time.perf_counter() - t0) * 1e3)
    m.close()
    return {"ms": statistics.median(ts[warm:]), "frames": sum(lens)}


def child_push(n, T=4):
    """{ms}: one push_any of n x T, window full, positions 72 + 5 s"""
    import numpy as np
    m = _model()
    rng = np.random.default_rng(n * 100 + T)
    warm, reps = 4, 10

    def codes(k, t):
        return rng.integers(0, 2048, size=(k, t, 16)).astype(np.int32)

    assert m.codec_mstream_begin(n, 4096) == 0
    assert m.codec_mstream_push(np.arange(n), codes(n, 72)) is not None      # fills the attention window
    for s in range(1, n):
        assert m.codec_mstream_push([s], codes(1, 5 * s)) is not None
    ts = []
    for _ in range(warm + reps):
        c = codes(n, T)
        t0 = time.perf_counter()
        o = m.codec_mstream_push_any(np.arange(n), c)
        ts.append((time.perf_counter() - t0) * 1e3)
        assert o is not None
    m.close()
    return {"ms": statistics.median(ts[warm:])}


def child_vc(mode, nb=8, frames=128, chunk=4):
    import numpy as np
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model()
    m.set_params(max_tokens=frames, fixed=frames, seed=42, **DEFAULT)
    if mode == "single_stream":
        nb = 1
    prompts = [prompt_ids("p128", seed=1234 + i) for i in range(nb)]
    vc = []
    for i in range(nb):        # bench.py --voice-clone --vc-codes
        r = np.random.default_rng(1234 + i + 7)
        codes = r.integers(0, 2048, size=(63, m.cfg.num_code_groups)).astype(np.int32)
        rids = [151644, 77091, 198] + r.integers(1000, 100000, size=20).tolist() + [151645, 198]
        vc.append((rids, codes, (r.standard_normal(m.cfg.talker_hidden) * 0.05).astype(np.float32)))
    rid, rc_, sv = [v[0] for v in vc], [v[1] for v in vc], [v[2] for v in vc]
    res = {}
    for it in range(2):        # the second request is the one reported
        t0 = time.perf_counter()
        if mode == "batch_stream":
            rc, audio = m.generate_voice_clone_batch_stream(prompts, rid, rc_, sv, ["english"] * nb, chunk_frames=chunk)
        elif mode == "batch":
            rc, audio = m.generate_voice_clone_batch(prompts, rid, rc_, sv, ["english"] * nb)
        else:
            a = m.generate_voice_clone_stream(prompts[0], rid[0], rc_[0], sv[0], "english", chunk_frames=chunk)
            rc, audio = (0 if a is not None else -1), [a]
        wall = time.perf_counter() - t0
        assert rc == 0 and all(a is not None for a in audio)
    secs = sum(len(a) for a in audio) / 24000.0
    res.update(audio_s_per_s=secs / wall, total_ms=wall * 1e3, codec_ms=float(m.c.perf_codec_ms),
               first_packet_ms=float(m.c.perf_first_packet_ms) if mode != "batch" else None)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vc_batch_stream_bench.txt"))
    ap.add_argument("--only", default="prime,push,vc,bench", help="comma list of prime, push, vc, bench")
    ap.add_argument("--append", action="store_true", help="append to --out instead of rewriting it")
    a = ap.parse_args()
    if a.child:
        kind = a.child[0]
        if kind == "prime":
            print(json.dumps(child_prime(a.child[1], int(a.child[2]))))
        elif kind == "push":
            print(json.dumps(child_push(int(a.child[1]))))
        else:
            print(json.dumps(child_vc(a.child[1])))
        return
    only = a.only.split(",")
    lines = [f"# tools/prof_vc_batch_stream.py --reps {a.reps} --only {a.only}: medians over {a.reps} fresh processes, "
             "synthetic 1.7B"]
    where = "the parent commit's build" if a.parent_lib else "this build"

    def say(s):
        lines.append(s)
        print(s, flush=True)
    if "prime" in only:
        for n in (8, 32):
            rows = {"ragged": [], "separate": [], "uniform": []}
            for _ in range(a.reps):
                rows["ragged"].append(spawn(["prime", "ragged", n]))
                rows["separate"].append(spawn(["prime", "separate", n], a.parent_lib))
                rows["uniform"].append(spawn(["prime", "uniform", n]))
            rg, sp, un = (med(rows[k], "ms") for k in ("ragged", "separate", "uniform"))
            fr = rows["ragged"][0]["frames"]
            say(f"prime n={n:2d} lengths 40..80 ({fr} frames, {80 * n} with padding): one ragged push {rg:8.3f} ms "
                f"({each(rows['ragged'], 'ms')})   {n} push_any on {where} {sp:8.3f} ms ({each(rows['separate'], 'ms')})"
                f"   ratio {sp / rg:.2f}x   uniform push of {n} x 80 {un:8.3f} ms ({each(rows['uniform'], 'ms')})   "
                f"ragged / uniform {rg / un:.3f}")
    if "push" in only:
        for n in (8, 32):
            rows = {"parent": [], "this": []}
            for _ in range(a.reps):
                rows["parent"].append(spawn(["push", n], a.parent_lib))
                rows["this"].append(spawn(["push", n]))
            p, t = med(rows["parent"], "ms"), med(rows["this"], "ms")
            say(f"push n={n:2d} T=4 window full, positions 72 + 5 s, push_any: {where} {p:7.3f} ms "
                f"({each(rows['parent'], 'ms')})   this build {t:7.3f} ms ({each(rows['this'], 'ms')})   "
                f"{100 * (t / p - 1):+.1f} %")
    if "vc" in only:
        plan = ["batch_stream", "batch", "single_stream"]
        rows = {p: [] for p in plan}
        for _ in range(a.reps):
            for p in plan:
                rows[p].append(spawn(["vc", p]))
        for p in plan:
            r = rows[p]
            what = "batch 1" if p == "single_stream" else "batch 8"
            fp = f"first packet {med(r, 'first_packet_ms'):7.2f} ms ({each(r, 'first_packet_ms', '{:.2f}')})   " \
                if p != "batch" else ""
            say(f"vc {p:13s} {what}, 63 reference frames, 128 frames, chunk 4: {fp}{med(r, 'audio_s_per_s'):7.1f} "
                f"audio-s/s ({each(r, 'audio_s_per_s', '{:.1f}')})   codec {med(r, 'codec_ms'):7.1f} ms of "
                f"{med(r, 'total_ms'):7.1f} ms")
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
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
