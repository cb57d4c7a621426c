#!/usr/bin/env python3
"""Batch streaming on the synthetic 1.7B model (measurement tool).

  python3 tools/prof_batch_stream.py [--reps 3] [--out profiles/batch_stream_bench.txt]

Every figure is the median over --reps fresh processes (one child process per
repetition and quantity; the two sides of a comparison alternate, one after
the other inside each repetition).

  push   one multi-stream push of n streams x T frames (qwen_tts_codec_mstream_push)
         against n pushes of T frames one after another through the single
         exact stream (qwen_tts_codec_stream_push): host wall, ms, the median
         over 10 pushes in the steady state (past the first frames)
  gen    qwen_tts_generate_batch_stream at batch 8 and 32, 128 frames,
         chunk_frames 4: first packet (ms), audio-s/s; beside
         qwen_tts_generate_batch at the same batch and qwen_tts_generate_stream
         at batch 1
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
    md = ensure_model(os.path.join(os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models"), "1.7b"), "1.7b")
    return qtts.QwenTTS(md)


def child_push(n, T):
    """{multi_ms, seq_ms}: one push of n x T against n single pushes of T"""
    import numpy as np
    m = _model()
    rng = np.random.default_rng(n * 100 + T)
    warm, reps = 4, 10
    codes = rng.integers(0, 2048, size=(n, (warm + reps) * T, 16)).astype(np.int32)
    pre = rng.integers(0, 2048, size=(n, 72, 16)).astype(np.int32)     # fills the attention window first
    out = {}
    for side in ("multi", "seq", "multi", "seq"):      # alternate; the second round of each is kept
        ts = []
        if side == "multi":
            assert m.codec_mstream_begin(n, 4096) == 0
            assert m.codec_mstream_push(np.arange(n), pre) is not None
            for k in range(warm + reps):
                c = np.ascontiguousarray(codes[:, k * T:(k + 1) * T])
                t0 = time.perf_counter()
                o = m.codec_mstream_push(np.arange(n), c)
                ts.append((time.perf_counter() - t0) * 1e3)
                assert o is not None
        else:
            # the single stream holds one state: n utterances one after another
            # means each push restarts from another utterance's position, which
            # the parent cannot do either; what is timed is its cost per push
            import ctypes as C
            L = __import__("qtts").lib()
            assert L.qwen_tts_codec_stream_begin(m.ctx, 4096) == 0
            o = np.zeros(72 * 1920, np.float32)
            c = np.ascontiguousarray(pre[0])
            assert L.qwen_tts_codec_stream_push(m.ctx, c.ctypes.data_as(C.POINTER(C.c_int)), 72,
                                                o.ctypes.data_as(C.POINTER(C.c_float))) == 72 * 1920
            for k in range(warm + reps):
                t0 = time.perf_counter()
                for s in range(n):
                    c = np.ascontiguousarray(codes[s, k * T:(k + 1) * T])
                    r = L.qwen_tts_codec_stream_push(m.ctx, c.ctypes.data_as(C.POINTER(C.c_int)), T,
                                                     o.ctypes.data_as(C.POINTER(C.c_float)))
                    assert r == T * 1920
                ts.append((time.perf_counter() - t0) * 1e3)
                if (k + 1) * T * n > 3900:
                    break
        out[side + "_ms"] = statistics.median(ts[warm:]) if len(ts) > warm else statistics.median(ts)
    m.close()
    return out


def child_gen(mode, batch, frames=128, chunk=4):
    """{first_packet_ms, total_ms, audio_s_per_s} of one call after one warm-up call"""
    from oracle_py import DEFAULT
    from synth_model import prompt_ids
    m = _model()
    m.set_params(max_tokens=4096, fixed=frames, seed=42, **DEFAULT)
    ids = [prompt_ids("p128", seed=1234 + b) for b in range(batch)]
    res = None
    for _ in range(2):
        t0 = time.perf_counter()
        if mode == "batch_stream":
            rc, audio = m.generate_batch_stream(ids, ["aiden"] * batch, ["english"] * batch, chunk_frames=chunk)
        elif mode == "batch":
            rc, audio = m.generate_batch(ids, ["aiden"] * batch, ["english"] * batch)
        else:
            rc, audio = 0, [m.generate_stream(ids[0], "aiden", "english", chunk_frames=chunk)]
        wall = time.perf_counter() - t0
        assert rc == 0 and all(a is not None for a in audio)
        secs = sum(len(a) for a in audio) / 24000.0
        res = {"first_packet_ms": float(m.c.perf_first_packet_ms) if mode != "batch" else None,
               "total_ms": wall * 1e3, "audio_s_per_s": secs / wall, "codec_ms": float(m.c.perf_codec_ms)}
    m.close()
    return res


def spawn(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args],
                       capture_output=True, text=True, timeout=900)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_stream_bench.txt"))
    ap.add_argument("--skip-gen", action="store_true")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "push":
            print(json.dumps(child_push(int(a.child[1]), int(a.child[2]))))
        else:
            print(json.dumps(child_gen(a.child[1], int(a.child[2]))))
        return
    lines = [f"# tools/prof_batch_stream.py --reps {a.reps}: medians over {a.reps} fresh processes, synthetic 1.7B"]
    for n in (8, 32, 64):
        for T in (1, 4):
            rows = [spawn("push", n, T) for _ in range(a.reps)]
            mu, sq = med(rows, "multi_ms"), med(rows, "seq_ms")
            lines.append(f"push n={n:2d} T={T}: multi-stream {mu:8.2f} ms   {n} single pushes {sq:8.2f} ms   "
                         f"ratio {sq / mu:5.2f}x   ({mu / (n * T):.3f} ms per stream-frame)")
            print(lines[-1], flush=True)
    if not a.skip_gen:
        plan = [("stream", 1), ("batch_stream", 8), ("batch", 8), ("batch_stream", 32), ("batch", 32)]
        rows = {p: [] for p in plan}
        for _ in range(a.reps):
            for p in plan:                     # alternating: every quantity once per repetition
                rows[p].append(spawn("gen", *p))
        for p in plan:
            fp = med(rows[p], "first_packet_ms")
            lines.append(f"gen {p[0]:12s} batch {p[1]:2d} 128 frames chunk 4: first packet "
                         f"{'   n/a' if fp != fp else f'{fp:6.2f}'} ms   {med(rows[p], 'audio_s_per_s'):7.1f} audio-s/s   "
                         f"codec {med(rows[p], 'codec_ms'):7.1f} ms of {med(rows[p], 'total_ms'):7.1f} ms")
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
