#!/usr/bin/env python3
"""Codec time in the four precision modes -- exact, convs-bf16
(qwen_tts_set_codec_precision), linears-bf16 (qwen_tts_set_codec_linear_precision),
both -- and this build's exact / convs-bf16 modes against a parent build, on the
synthetic 1.7B model.  The sibling of codec_bf16_bench.py, with the same method:
every side in fresh child processes (QTTS_LIB selects the library), the sides
alternating, `--runs` children per side; a child reports the median of `--reps`
timed calls after one warm-up call per shape, the table the median of the
children.  Times are host clocks around calls that end in a device synchronise:

  codec B x 128   qtts_dev_codec_multi: B stateless decodes of 128 frames (random codes)
  push N x 4      one multi-stream push of 4 frames on each of N streams
  push 1 x 1      one single-stream push of 1 frame (the first-packet case)
  quality         each mode against exact, one 128-frame decode: MSE, max |d|, SNR
  sha             sha256 of that decode's bytes (equal between a build and its parent in the parent's modes)

  python tools/codec_lin_bf16_bench.py [--parent-lib PATH] [--runs 3] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, "qwen3-tts-c_amd")]

BATCHES, PUSHES, FRAMES = (1, 8, 32), (8, 32), 128
MODES = {"exact": (0, 0), "convs": (1, 0), "linears": (0, 1), "both": (1, 1)}   # (conv, linear) precision


def child(mode, reps):
    import numpy as np
    import qtts
    from synth_model import ensure_model
    root = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    L = qtts.lib()
    m = qtts.QwenTTS(ensure_model(os.path.join(root, "1.7b"), "1.7b", seed=0))
    conv, linear = MODES[mode]
    w0 = int(L.qtts_dev_bytes(C.c_void_p(m.c.hip), 0))
    m.set_codec_precision(conv)
    if linear:
        m.set_codec_linear_precision(linear)
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.qtts_dev_codec_multi.argtypes = [C.c_void_p, C.c_int, C.POINTER(ip), ip, ip, C.POINTER(fp), ip]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 2048, size=(max(BATCHES), FRAMES, 16)).astype(np.int32)

    def multi(n):
        hc = (ip * n)(*[codes[i].ctypes.data_as(ip) for i in range(n)])
        T, audio, ns = (C.c_int * n)(*[FRAMES] * n), (fp * n)(), (C.c_int * n)()
        t0 = time.perf_counter()
        rc = L.qtts_dev_codec_multi(m.c.hip, n, hc, None, T, audio, ns)
        dt = time.perf_counter() - t0
        assert rc == 0 and all(ns[i] == FRAMES * 1920 for i in range(n)), rc
        for i in range(n):
            libc.free(C.cast(audio[i], C.c_void_p))
        return dt * 1e3

    def push(n, k):
        t0 = time.perf_counter()
        o = m.codec_mstream_push(list(range(n)), codes[:n, 4 * k:4 * k + 4])
        dt = time.perf_counter() - t0
        assert o is not None
        return dt * 1e3

    out1 = np.zeros(1920, np.float32)

    def push1(k):
        t0 = time.perf_counter()
        got = L.qwen_tts_codec_stream_push(m.ctx, codes[0, k:k + 1].ctypes.data_as(ip), 1, out1.ctypes.data_as(fp))
        dt = time.perf_counter() - t0
        assert got == 1920, got
        return dt * 1e3

    res = {"mode": mode, "weight_bytes_before": w0}
    for n in BATCHES:
        multi(n)
        res[f"codec_{n}x{FRAMES}_ms"] = statistics.median(multi(n) for _ in range(reps))
    for n in PUSHES:
        assert m.codec_mstream_begin(n, 4 * (reps + 2)) == 0
        push(n, 0)
        res[f"push_{n}x4_ms"] = statistics.median(push(n, k + 1) for k in range(reps))
    assert L.qwen_tts_codec_stream_begin(m.ctx, reps + 2) == 0
    push1(0)
    res["push_1x1_ms"] = statistics.median(push1(k + 1) for k in range(reps))
    a = m.codec_decode(codes[0])
    res["sha"] = hashlib.sha256(a.tobytes()).hexdigest()[:16]
    res["weight_bytes"] = int(L.qtts_dev_bytes(C.c_void_p(m.c.hip), 0))
    if mode != "exact":
        m.set_codec_precision(0)
        if linear:
            m.set_codec_linear_precision(0)
        a, e = a.astype(np.float64), m.codec_decode(codes[0]).astype(np.float64)
        mse = float(np.mean((a - e) ** 2))
        res.update(quality_mse=mse, quality_maxabs=float(np.abs(a - e).max()),
                   quality_snr_db=float(10 * np.log10(np.mean(e ** 2) / mse)))
    m.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib, mode, reps):
    env = dict(os.environ)
    for k in ("QTTS_LIB", "QTTS_HIP_CODEC", "QTTS_HIP_CODEC_LIN"):
        env.pop(k, None)
    if lib:
        env["QTTS_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(reps)], env=env,
                       capture_output=True, text=True, timeout=600)
    out = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not out:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child ({lib or 'this build'}, {mode}) failed ({r.returncode})")
    return json.loads(out[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    sides = [(mode, None, mode) for mode in MODES]
    if a.parent_lib:
        sides = [("parent exact", a.parent_lib, "exact"), ("parent convs", a.parent_lib, "convs")] + sides
    got = {s[0]: [] for s in sides}
    for _ in range(a.runs):
        for name, lib, mode in sides:           # alternating sides
            got[name].append(run_child(lib, mode, a.reps))
            print(name, json.dumps(got[name][-1]), flush=True)
    keys = [k for k in got["exact"][0] if k.endswith("_ms")]
    med = lambda n, k: statistics.median(r[k] for r in got[n])
    lines = [f"# tools/codec_lin_bf16_bench.py: synthetic 1.7B, medians of {a.runs} fresh processes per side "
             f"(each the median of {a.reps} calls), sides alternating; ms (min .. max of the processes)"]
    for k in keys:
        lines.append(k)
        for n in got:
            v = [r[k] for r in got[n]]
            lines.append(f"    {n:14s}{statistics.median(v):10.3f} ({min(v):7.3f}..{max(v):7.3f})   / exact "
                         f"{statistics.median(v) / med('exact', k):.3f}")
    for n in got:
        q = got[n][0]
        line = f"{n:14s} sha {q['sha']}  weight bytes {q['weight_bytes_before']} -> {q['weight_bytes']}"
        if "quality_mse" in q:
            line += (f"  against exact: mse {q['quality_mse']:.3e}  max |d| {q['quality_maxabs']:.3e}  "
                     f"snr {q['quality_snr_db']:.1f} dB")
        lines.append(line)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
