#!/usr/bin/env python3
"""Talker prefill time in the two prefill attention precisions
(qwen_tts_set_prefill_attention_precision) and this build's exact mode against a
parent build, on the synthetic 1.7B model, by the method of
tools/prefill_bf16_bench.py: seeded N(0, 0.25) embedding rows through
qwen_tts_talker_prefill (host rows in, the last row's hidden out, synchronous),
every side in fresh child processes (QTTS_LIB selects the library), the sides
alternating, `--runs` children per side.  A child runs the four combinations of
cache type (fp32 | bf16) and prefill precision (exact | bf16) on one context
and reports, per combination and row count, the median of `--reps` timed calls
after one warm-up call, the sha256 of the hidden's bytes and the k_attn_tileh
launches of the timed calls.  `--kernels` times the two tiled attention kernels
on their own through the kernel-level entries (prep 0: q ready, caches filled;
events around the one call, which holds a 16-byte table copy and two stream
waits besides the launch), 16 query heads, 8 kv heads, HD 128, one segment.

  python tools/prefill_attn_bf16_bench.py [--parent-lib PATH] [--runs 3] [--reps 3] [--out FILE] [--kernels]
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

ROWS = (256, 512, 1024, 4000)
COMBOS = [(kv, pp) for kv in ("fp32", "bf16") for pp in ("exact", "bf16")]


def child(mode, reps):
    import numpy as np
    import qtts
    from synth_model import ensure_model
    root = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    L = qtts.lib()
    m = qtts.QwenTTS(ensure_model(os.path.join(root, "1.7b"), "1.7b", seed=0))
    if mode == "on":
        m.set_prefill_attention_precision("bf16")
    count = (lambda: qtts.Kernels.attn_tileh_launches()) if hasattr(L, "qtts_hip_attn_tileh_launches") else (lambda: 0)
    res = {"mode": mode}
    for kv, pp in COMBOS:
        m.set_kv_cache(kv)
        m.set_prefill_precision(pp)
        for n in ROWS:
            e = (np.random.default_rng(n).standard_normal((n, m.cfg.talker_hidden)) * 0.5).astype(np.float32)
            h = m.prefill(e)
            c0, ts = count(), []
            for _ in range(reps):
                t0 = time.perf_counter()
                h = m.prefill(e)
                ts.append((time.perf_counter() - t0) * 1e3)
            res[f"{kv}/{pp}/{n}"] = dict(ms=statistics.median(ts), sha=hashlib.sha256(h.tobytes()).hexdigest()[:16],
                                         launches=count() - c0, hidden=h.astype(float).tolist() if n == 1024 else None)
    m.close()
    print("RESULT " + json.dumps(res), flush=True)


def kernels(reps):
    """the two attention kernels alone: ms per launch, median of `reps` after one warm-up"""
    import torch
    import qtts
    NH, KV, HD = 16, 8, 128
    lines = ["# the tiled attention kernels alone (kernel-level entries, prep 0), NH 16, KV 8, HD 128, one segment from "
             f"position 0; events around one call; median of {reps} after one warm-up; ms",
             "rows   cache  k_attn_tile  k_attn_tileh  ratio"]
    for n in (1024, 4000):
        g = torch.Generator(device="cuda:0").manual_seed(n)
        q = torch.randn((n, NH * HD), generator=g, device="cuda:0")
        k32, v32 = (torch.randn((1, n, KV * HD), generator=g, device="cuda:0") for _ in range(2))
        seg = torch.tensor([[0, 0, 0, n]], dtype=torch.int32, device="cuda:0")
        out = torch.empty((n, NH * HD), device="cuda:0")
        for name, kc, vc, dt in (("fp32", k32, v32, 0),
                                 ("bf16", k32.bfloat16().view(torch.int16), v32.bfloat16().view(torch.int16), 1)):
            ms = {}
            for fn in (qtts.Kernels.attn_tiled, qtts.Kernels.attn_tiled_bf16):
                ts = []
                for i in range(reps + 1):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    assert fn(out, q, NH * HD, kc, vc, None, None, None, None, seg, 1, NH, KV, HD, n, 1, n, 1e-6, 0, dt, 0)
                    b.record()
                    torch.cuda.synchronize()
                    ts.append(a.elapsed_time(b))
                ms[fn.__name__] = statistics.median(ts[1:])
            lines.append(f"{n:<7d}{name:7s}{ms['attn_tiled']:11.3f}{ms['attn_tiled_bf16']:14.3f}"
                         f"{ms['attn_tiled_bf16'] / ms['attn_tiled']:7.3f}")
    return lines


def run_child(lib, mode, reps):
    env = dict(os.environ)
    for k in ("QTTS_LIB", "QTTS_HIP_PREFILL", "QTTS_HIP_PREFILL_ATTN", "QTTS_HIP_KV"):
        env.pop(k, None)
    if lib:
        env["QTTS_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(reps)], env=env,
                       capture_output=True, text=True, timeout=900)
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
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    sides = [("off", None, "off"), ("on", None, "on")]
    if a.parent_lib:
        sides.insert(0, ("parent", a.parent_lib, "off"))
    got = {s[0]: [] for s in sides}
    for _ in range(a.runs):
        for name, lib, mode in sides:           # alternating sides
            got[name].append(run_child(lib, mode, a.reps))
            print(name, " ".join(f"{k}:{v['ms']:.2f}" for k, v in got[name][-1].items() if k != "mode"), flush=True)
    med = lambda s, k: statistics.median(r[k]["ms"] for r in got[s])
    lines = [f"# tools/prefill_attn_bf16_bench.py: qwen_tts_talker_prefill, synthetic 1.7B, one slot; per side {a.runs} "
             f"fresh processes, alternating; each figure the median of {a.reps} calls after one warm-up; ms",
             "# off / on: this build with the prefill attention switch exact / bf16; cache/prefill: the KV cache type "
             "and the prefill (projection) precision",
             f"{'cache/prefill/rows':21s}" + "".join(f"{s + ' (processes)':30s}{'median':>9s}   " for s in got) + "ratios"]
    keys = [f"{kv}/{pp}/{n}" for kv, pp in COMBOS for n in ROWS]
    for k in keys:
        line = f"{k:21s}"
        for s in got:
            line += "".join(f"{r[k]['ms']:9.3f}" for r in got[s]).ljust(30) + f"{med(s, k):9.3f}   "
        if "parent" in got:
            line += f"off / parent {med('off', k) / med('parent', k):.3f}  "
        line += f"on / off {med('on', k) / med('off', k):.3f}  k_attn_tileh launches {got['on'][0][k]['launches']}"
        lines.append(line)
    shas = {s: [tuple(r[k]["sha"] for k in keys) for r in got[s]] for s in got}
    for s in got:
        lines.append(f"{s:7s} hidden sha256 per line: {' '.join(shas[s][0])}"
                     f"   (the side's processes agree: {len(set(shas[s])) == 1})")
    if "parent" in got:
        lines.append(f"switch-off hidden bytes equal the parent's on every line: {shas['off'][0] == shas['parent'][0]}")
    lines.append(f"switch-on differs from switch-off on every line: {all(x != y for x, y in zip(shas['on'][0], shas['off'][0]))}")
    import numpy as np
    for kv in ("fp32", "bf16"):
        hb, he = (np.array(got[s][0][f"{kv}/exact/1024"]["hidden"]) for s in ("on", "off"))
        lines.append(f"1024 rows, {kv} cache, exact projections, hidden on against off: |d| / |off| = "
                     f"{np.linalg.norm(hb - he) / np.linalg.norm(he):.3e}")
    if a.kernels:
        lines += kernels(5)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
