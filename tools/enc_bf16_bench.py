#!/usr/bin/env python3
"""The voice-clone audio encoders in the two encoder precisions
(qwen_tts_set_encoder_precision) and this build's exact mode against a parent
build, on the synthetic 1.7B model with 5 s of seeded reference audio per
utterance (synth_model.ref_wave), at batch 1 and batch 8.  Every side runs in
fresh child processes (QTTS_LIB selects the library), the sides alternating,
`--runs` children per side.  A child reports, per batch:

  encode        wall ms of speaker_embed + encode_audio (host waveforms in, host
                x-vectors and codes out, both synchronous), median of `--reps`
                calls after one warm-up
  first packet  perf_first_packet_ms of generate_voice_clone_audio_batch_stream
                (8 frames, chunks of 4; the encode is inside it), second request
  the x-vectors, the codes, and the sha256 of both

and the parent process writes the medians, each side's spread, the bf16
x-vector's cosine against exact and the share of the 16-codebook codes equal
to exact mode's.

  python tools/enc_bf16_bench.py [--parent-lib PATH] [--runs 3] [--reps 5] [--out FILE]
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
sys.path[:0] = [HERE, os.path.join(ROOT, "qwen3-tts-c_amd"), os.path.join(ROOT, "tests")]

BATCHES = (1, 8)


def child(mode, reps):
    import numpy as np
    import qtts
    from oracle_py import DEFAULT
    from synth_model import ensure_model, prompt_ids, ref_wave
    root = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    m = qtts.QwenTTS(ensure_model(os.path.join(root, "1.7b"), "1.7b", seed=0))
    assert m.encoders_available() == 3
    if mode == "bf16":
        m.set_encoder_precision("bf16")
    count = qtts.Kernels.econvh_launches if hasattr(qtts.lib(), "qtts_hip_econvh_launches") else (lambda: 0)
    m.set_params(max_tokens=8, fixed=8, seed=42, **DEFAULT)
    res = {"mode": mode}
    for nb in BATCHES:
        wavs = [ref_wave(1234 + i + 7, 5.0) for i in range(nb)]
        prompts = [prompt_ids("p128", seed=1234 + i) for i in range(nb)]
        rids = [[151644, 77091, 198] + np.random.default_rng(i).integers(1000, 100000, size=20).tolist() + [151645, 198]
                for i in range(nb)]
        c0, ts = count(), []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            xv = m.speaker_embed(wavs)
            codes = m.encode_audio(wavs)
            ts.append((time.perf_counter() - t0) * 1e3)
        for _ in range(2):
            rc, audio = m.generate_voice_clone_audio_batch_stream(prompts, wavs, rids, ["english"] * nb, chunk_frames=4)
            assert rc == 0 and all(a is not None for a in audio)
        h = hashlib.sha256(xv.tobytes() + b"".join(c.tobytes() for c in codes)).hexdigest()[:16]
        res[str(nb)] = dict(encode_ms=statistics.median(ts[1:]), first_packet_ms=float(m.c.perf_first_packet_ms), sha=h,
                            launches=count() - c0, xv=xv.astype(float).tolist(), codes=[c.tolist() for c in codes])
    m.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib, mode, reps):
    env = dict(os.environ)
    for k in ("QTTS_LIB", "QTTS_HIP_ENC"):
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    import numpy as np
    sides = [("exact", None, "exact"), ("bf16", None, "bf16")]
    if a.parent_lib:
        sides.insert(0, ("parent", a.parent_lib, "exact"))
    got = {s[0]: [] for s in sides}
    for _ in range(a.runs):
        for name, lib, mode in sides:           # alternating sides
            got[name].append(run_child(lib, mode, a.reps))
            print(name, " ".join(f"b{nb}: {got[name][-1][str(nb)]['encode_ms']:.2f} / "
                                 f"{got[name][-1][str(nb)]['first_packet_ms']:.2f}" for nb in BATCHES), flush=True)
    lines = [f"# tools/enc_bf16_bench.py: synthetic 1.7B, 5 s of reference audio per utterance; per side {a.runs} fresh "
             f"processes, alternating; encode: speaker_embed + encode_audio, median of {a.reps} calls after one warm-up; "
             "first packet: generate_voice_clone_audio_batch_stream, second request; ms",
             "# parent: the parent commit's build; exact / bf16: this build with the encoder switch off / on",
             f"{'batch figure':24s}" + "".join(f"{s + ' (processes)':30s}{'median':>9s}{'spread':>8s}   " for s in got)
             + "ratios"]
    for nb in BATCHES:
        for fig in ("encode_ms", "first_packet_ms"):
            v = {s: [r[str(nb)][fig] for r in got[s]] for s in got}
            md = {s: statistics.median(v[s]) for s in got}
            line = f"{nb:<6d}{fig:18s}"
            for s in got:
                line += ("".join(f"{x:9.3f}" for x in v[s]).ljust(30) + f"{md[s]:9.3f}"
                         f"{(max(v[s]) - min(v[s])) / md[s] * 100:7.1f}%   ")
            if "parent" in got:
                line += f"exact / parent {md['exact'] / md['parent']:.3f}  "
            lines.append(line + f"bf16 / exact {md['bf16'] / md['exact']:.3f}")
    for nb in BATCHES:
        shas = {s: [r[str(nb)]["sha"] for r in got[s]] for s in got}
        lines.append(f"batch {nb}: x-vector + codes sha256 " + "  ".join(f"{s} {shas[s][0]}" for s in got)
                     + f"   (each side's processes agree: {all(len(set(v)) == 1 for v in shas.values())})"
                     + (f"   exact equals parent: {shas['exact'][0] == shas['parent'][0]}" if "parent" in got else ""))
        e, h = got["exact"][0][str(nb)], got["bf16"][0][str(nb)]
        cos = [float(np.dot(x, y) / (np.linalg.norm(x) * np.linalg.norm(y))) for x, y in zip(e["xv"], h["xv"])]
        ce, ch = np.concatenate([np.array(c) for c in e["codes"]]), np.concatenate([np.array(c) for c in h["codes"]])
        lines.append(f"batch {nb}: bf16 against exact: x-vector cosine min {min(cos):.6f} mean {np.mean(cos):.6f}; codes "
                     f"equal {np.mean(ce == ch) * 100:.1f} % of {ce.size} (codebook 0: {np.mean(ce[:, 0] == ch[:, 0]) * 100:.1f} "
                     f"%); k_econvh launches in the bf16 child {h['launches']}, in the exact child {e['launches']}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
