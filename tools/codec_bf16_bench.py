#!/usr/bin/env python3
"""Codec time in exact and bf16 precision (qwen_tts_set_codec_precision), and
this build's exact mode against a parent build, on the synthetic 1.7B model.

Every side runs in fresh child processes (QTTS_LIB selects the library), the
sides alternating, `--runs` children per side; a child reports the median of
`--reps` timed calls after one warm-up call per shape, the table the median of
the children.  Times are host clocks around calls that end in a device
synchronise:

  codec B x 128   qtts_dev_codec_multi: B stateless decodes of 128 frames (random codes)
  push N x 4      one multi-stream push of 4 frames on each of N streams
  quality         bf16 against exact waveform of one 128-frame decode: MSE, max |d|, SNR

  python tools/codec_bf16_bench.py [--parent-lib PATH] [--runs 3] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
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


def child(mode, reps):
    import numpy as np
    import qtts
    from synth_model import ensure_model
    root = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    L = qtts.lib()
    m = qtts.QwenTTS(ensure_model(os.path.join(root, "1.7b"), "1.7b", seed=0))
    if mode == "bf16":
        m.set_codec_precision("bf16")
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

    res = {"mode": mode}
    for n in BATCHES:
        multi(n)
        res[f"codec_{n}x{FRAMES}_ms"] = statistics.median(multi(n) for _ in range(reps))
    for n in PUSHES:
        assert m.codec_mstream_begin(n, 4 * (reps + 2)) == 0
        push(n, 0)
        res[f"push_{n}x4_ms"] = statistics.median(push(n, k + 1) for k in range(reps))
    if mode == "bf16":
        a = m.codec_decode(codes[0]).astype(np.float64)
        m.set_codec_precision("exact")
        e = m.codec_decode(codes[0]).astype(np.float64)
        mse = float(np.mean((a - e) ** 2))
        res.update(quality_mse=mse, quality_maxabs=float(np.abs(a - e).max()),
                   quality_snr_db=float(10 * np.log10(np.mean(e ** 2) / mse)), exact_rms=float(np.sqrt(np.mean(e ** 2))))
    m.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib, mode, reps):
    env = dict(os.environ)
    env.pop("QTTS_LIB", None)
    env.pop("QTTS_HIP_CODEC", None)
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
    sides = [("exact", None, "exact"), ("bf16", None, "bf16")]
    if a.parent_lib:
        sides.insert(0, ("parent", a.parent_lib, "exact"))
    got = {s[0]: [] for s in sides}
    for _ in range(a.runs):
        for name, lib, mode in sides:           # alternating sides
            got[name].append(run_child(lib, mode, a.reps))
            print(name, json.dumps(got[name][-1]), flush=True)
    keys = [k for k in got["exact"][0] if k.endswith("_ms")]
    lines = [f"# tools/codec_bf16_bench.py: synthetic 1.7B, medians of {a.runs} fresh processes per side "
             f"(each the median of {a.reps} calls), sides alternating; ms (min .. max of the processes)",
             f"{'':18s}" + "".join(f"{n:>30s}" for n in got)]
    for k in keys:
        row = f"{k:18s}"
        for n in got:
            v = [r[k] for r in got[n]]
            row += f"{statistics.median(v):12.3f} ({min(v):7.3f}..{max(v):7.3f})"
        lines.append(row)
    med = lambda n, k: statistics.median(r[k] for r in got[n])
    for k in keys:
        lines.append(f"bf16 / exact {k:18s} {med('bf16', k) / med('exact', k):.3f}"
                     + (f"   exact / parent {med('exact', k) / med('parent', k):.3f}" if a.parent_lib else ""))
    q = got["bf16"][0]
    lines.append(f"quality, bf16 against exact, one {FRAMES}-frame decode: mse {q['quality_mse']:.3e}  max |d| "
                 f"{q['quality_maxabs']:.3e}  snr {q['quality_snr_db']:.1f} dB  (exact rms {q['exact_rms']:.3e})")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
