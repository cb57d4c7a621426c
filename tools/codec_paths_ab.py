#!/usr/bin/env python3
"""The three codec decode paths (one-shot, single stream, multi-stream) on two
builds of the library: same bytes out, same kernel launches in the same order.

Every side runs in a fresh child process (QTTS_LIB selects its library).  A
child decodes fixed random codes on the synthetic tiny model with sliding
window 16 (and two pushes on the synthetic 1.7B, where the planner takes other
paths) and writes each case's raw float32 audio to <dir>/<case>.f32:

  full_T{1,17,150}    one-shot decode (150 > the 64-frame scratch floor: re-allocated)
  stream_p{1,3,7,16,23}  one begin, then pushes that cross the 16-frame chunk and the window
  stream_chunk40      begin with chunk 40, one push of 40 frames
  ms3_same4           3 streams, one push of 4 frames at one position
  ms3_ragged          counts (1, 5, 20): one stream crosses the window, two do not
  ms3_restored        reset of stream 1, save of stream 0 -> restore into stream 2, push of (2, 2, 2)
  ms17_T1             17 streams, one push of 1 frame
  big_stream_T1, big_ms8_T1   synthetic 1.7B: one single-stream push, one 8 x 1 multi-stream push

  python tools/codec_paths_ab.py --parent-lib PATH [--trace] [--out FILE] [--work DIR]

--parent-lib: the parent commit's library (`make VARIANT=_a` in a checkout of
it).  The bytes of every case must be equal between the two libraries.
--trace: each child once more under `rocprofv3 --kernel-trace` (nothing else
traced, no counters); the ordered (kernel, grid, workgroup) lists of every
case must be equal.  A case ends at a sentinel launch (k_expf_glibc with a
grid of its own) that the child puts between the cases, so the trace needs no
markers.  Memory copies and memsets are no kernels and are not in the trace.
"""
import argparse
import csv
import glob
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, "qwen3-tts-c_amd")]

SENTINEL = "k_expf_glibc"
SENTINEL_N0 = 256 * 7001          # case i ends at a sentinel of 256 * (7001 + i) threads
SENTINEL_MAX = 40                 # cases the sentinel's buffer covers


def child(out_dir):
    import ctypes as C
    import numpy as np
    import torch
    import qtts
    from synth_model import ensure_model
    root = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    L = qtts.lib()
    os.makedirs(out_dir, exist_ok=True)
    L.qtts_dev_codec_stream_begin_ex.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.qtts_dev_codec_stream_push_host.argtypes = [C.c_void_p, ip, C.c_int, fp]
    buf = torch.zeros(SENTINEL_N0 + 256 * SENTINEL_MAX, device="cuda")   # the sentinel reads and writes n floats of it
    done = []

    def case(name, audio):
        a = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).ravel() for x in audio]))
        assert a.size and np.isfinite(a).all() and len(done) < SENTINEL_MAX, name
        a.tofile(os.path.join(out_dir, name + ".f32"))
        qtts.Kernels.expf_glibc(buf, buf, SENTINEL_N0 + 256 * len(done))   # (the kernel reads n floats: grid = n)
        torch.cuda.synchronize()
        done.append(name)
        print(f"CASE {name} {a.size * 4} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)

    def codes(rng, *shape):
        return rng.integers(0, 2048, size=shape + (16,)).astype(np.int32)

    def stream_push(m, c):
        o = np.zeros(len(c) * 1920, np.float32)
        k = L.qtts_dev_codec_stream_push_host(m.c.hip, c.ctypes.data_as(ip), len(c), o.ctypes.data_as(fp))
        assert k == len(o), k
        return o

    rng = np.random.default_rng(20240521)
    m = qtts.QwenTTS(ensure_model(os.path.join(root, "tiny_c_window16"), "tiny", seed=0, overrides={"c_window": 16}))
    for T in (1, 17, 150):
        case(f"full_T{T}", [m.codec_decode(codes(rng, T))])
    assert L.qtts_dev_codec_stream_begin_ex(m.c.hip, 256, 0) == 0
    for T in (1, 3, 7, 16, 23):
        case(f"stream_p{T}", [stream_push(m, codes(rng, T))])
    assert L.qtts_dev_codec_stream_begin_ex(m.c.hip, 256, 40) == 0
    case("stream_chunk40", [stream_push(m, codes(rng, 40))])
    assert m.codec_mstream_begin(3, 64) == 0
    case("ms3_same4", m.codec_mstream_push([0, 1, 2], codes(rng, 3, 4)))
    case("ms3_ragged", m.codec_mstream_push_ragged([0, 1, 2], [codes(rng, t) for t in (1, 5, 20)]))
    assert m.codec_mstream_reset(1) == 0
    snap = m.codec_mstream_save(0)
    assert snap and m.codec_mstream_restore(2, snap) == 0
    case("ms3_restored", m.codec_mstream_push_any([0, 1, 2], codes(rng, 3, 2)))
    m.codec_snapshot_free(snap)
    assert m.codec_mstream_begin(17, 16) == 0
    case("ms17_T1", m.codec_mstream_push(list(range(17)), codes(rng, 17, 1)))
    m.close()
    m = qtts.QwenTTS(ensure_model(os.path.join(root, "1.7b"), "1.7b", seed=0))
    assert L.qtts_dev_codec_stream_begin_ex(m.c.hip, 64, 0) == 0
    case("big_stream_T1", [stream_push(m, codes(rng, 1))])
    assert m.codec_mstream_begin(8, 16) == 0
    case("big_ms8_T1", m.codec_mstream_push(list(range(8)), codes(rng, 8, 1)))
    m.close()
    print("CASES " + " ".join(done), flush=True)


def run_child(lib, out_dir, trace_dir=None):
    env = dict(os.environ)
    env.pop("QTTS_LIB", None)
    if lib:
        env["QTTS_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", out_dir]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "-f", "csv", "-d", trace_dir, "-o", "run", "--"] + cmd
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    names = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("CASES ")]
    if r.returncode != 0 or not names:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child on {lib or 'this build'} failed ({r.returncode})")
    print(f"ran {len(names[0])} cases on {lib or 'this build'}{' under rocprofv3' if trace_dir else ''}", flush=True)
    return names[0]


def launches(trace_dir, cases):
    """{case: [(kernel, grid xyz, workgroup xyz)]} of a child's kernel trace"""
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit(f"{trace_dir}: expected one kernel trace, found {paths}")
    with open(paths[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    out, cur, i = {}, [], 0
    for r in rows:
        key = (r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"),
               tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"))
        if SENTINEL in key[0] and i < len(cases) and key[1][0] == SENTINEL_N0 + 256 * i:
            out[cases[i]] = cur
            cur, i = [], i + 1
        else:
            cur.append(key)
    if i != len(cases):
        raise SystemExit(f"{trace_dir}: {i} of {len(cases)} sentinels found")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--work", default=os.path.join(ROOT, "ab_out", "codec_paths"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.parent_lib:
        raise SystemExit("--parent-lib PATH is required")
    sides = {"parent": a.parent_lib, "branch": None}
    cases = {s: run_child(lib, os.path.join(a.work, s)) for s, lib in sides.items()}
    if cases["parent"] != cases["branch"]:
        raise SystemExit("the two sides ran different cases")
    names = cases["branch"]
    lines, bad = [f"# tools/codec_paths_ab.py: parent library {a.parent_lib} against this build"], 0
    traces = None
    if a.trace:
        traces = {}
        for s, lib in sides.items():
            td = os.path.join(a.work, s + "_trace")
            run_child(lib, os.path.join(a.work, s + "_traced"), td)
            traces[s] = launches(td, names)
    for n in names:
        pb, bb = (open(os.path.join(a.work, s, n + ".f32"), "rb").read() for s in ("parent", "branch"))
        same = pb == bb
        line = f"{n:16s} {len(bb):9d} bytes  {'equal' if same else 'DIFFERENT'}"
        if traces:
            tp, tb = traces["parent"][n], traces["branch"][n]
            tsame = tp == tb
            line += f"   launches {len(tp):5d} / {len(tb):5d}  {'identical' if tsame else 'DIFFERENT'}"
            if not tsame:
                k = next((i for i, (x, y) in enumerate(zip(tp, tb)) if x != y), min(len(tp), len(tb)))
                line += f" (first at {k}: {tp[k] if k < len(tp) else None} / {tb[k] if k < len(tb) else None})"
            same = same and tsame
        bad += not same
        lines.append(line)
        print(line, flush=True)
    lines.append("verdict: " + ("every case byte-equal" + (" and launch-identical" if traces else "") if not bad
                                else f"{bad} case(s) differ"))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
