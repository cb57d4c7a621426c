#!/usr/bin/env python3
"""Talker prefill time in the two prefill precisions (qwen_tts_set_prefill_precision)
and this build's exact mode against a parent build, on the synthetic 1.7B model.
The method of profiles/attn_tile_bench.txt: seeded N(0, 0.25) embedding rows
through qwen_tts_talker_prefill (host rows in, the last row's hidden out,
synchronous), every side in fresh child processes (QTTS_LIB selects the
library), the sides alternating, `--runs` children per side; a child reports,
per row count, the median of `--reps` timed calls after one warm-up call, the
sha256 of the hidden's bytes and the k_pgemmh launches of the timed calls.

  python tools/prefill_bf16_bench.py [--parent-lib PATH] [--runs 3] [--reps 3] [--out FILE]
"""
import argparse
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

ROWS = (64, 128, 256, 512, 1024, 4000)


def child(mode, reps):
    import numpy as np
    import qtts
    from synth_model import ensure_model
    root = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    L = qtts.lib()
    m = qtts.QwenTTS(ensure_model(os.path.join(root, "1.7b"), "1.7b", seed=0))
    if mode == "bf16":
        m.set_prefill_precision("bf16")
    count = (lambda: qtts.Kernels.pgemmh_launches()) if hasattr(L, "qtts_hip_pgemmh_launches") else (lambda: 0)
    res = {"mode": mode}
    for n in ROWS:
        e = (np.random.default_rng(n).standard_normal((n, m.cfg.talker_hidden)) * 0.5).astype(np.float32)
        h = m.prefill(e)
        c0, ts = count(), []
        for _ in range(reps):
            t0 = time.perf_counter()
            h = m.prefill(e)
            ts.append((time.perf_counter() - t0) * 1e3)
        res[str(n)] = dict(ms=statistics.median(ts), sha=hashlib.sha256(h.tobytes()).hexdigest()[:16],
                           launches=count() - c0, hidden=h.astype(float).tolist() if n == 256 else None)
    m.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib, mode, reps):
    env = dict(os.environ)
    for k in ("QTTS_LIB", "QTTS_HIP_PREFILL"):
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
    ap.add_argument("--reps", type=int, default=3)
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
            print(name, " ".join(f"{n}:{got[name][-1][str(n)]['ms']:.3f}" for n in ROWS), flush=True)
    med = lambda s, n: statistics.median(r[str(n)]["ms"] for r in got[s])
    lines = [f"# tools/prefill_bf16_bench.py: qwen_tts_talker_prefill, synthetic 1.7B, one slot; per side {a.runs} fresh "
             f"processes, alternating; each figure the median of {a.reps} calls after one warm-up; ms",
             "rows   " + "".join(f"{s + ' (processes)':32s}{'median':>9s}   " for s in got) + "ratios"]
    for n in ROWS:
        line = f"{n:<7d}"
        for s in got:
            line += "".join(f"{r[str(n)]['ms']:9.3f}" for r in got[s]).ljust(32) + f"{med(s, n):9.3f}   "
        if "parent" in got:
            line += f"exact / parent {med('exact', n) / med('parent', n):.3f}  "
        line += f"bf16 / exact {med('bf16', n) / med('exact', n):.3f}  k_pgemmh launches {got['bf16'][0][str(n)]['launches']}"
        lines.append(line)
    shas = {s: [tuple(r[str(n)]["sha"] for n in ROWS) for r in got[s]] for s in got}
    for s in got:
        lines.append(f"{s:7s} hidden sha256 per row count: {' '.join(shas[s][0])}"
                     f"   (the side's processes agree: {len(set(shas[s])) == 1})")
    if "parent" in got:
        lines.append(f"exact mode's hidden bytes equal the parent's at every row count: {shas['exact'][0] == shas['parent'][0]}")
    lines.append(f"bf16 differs from exact at every row count: {all(x != y for x, y in zip(shas['bf16'][0], shas['exact'][0]))}")
    import numpy as np
    hb, he = (np.array(got[s][0]["256"]["hidden"]) for s in ("bf16", "exact"))
    lines.append(f"256 rows, hidden bf16 against exact: |d| / |exact| = {np.linalg.norm(hb - he) / np.linalg.norm(he):.3e}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
