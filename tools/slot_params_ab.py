#!/usr/bin/env python3
"""What per-slot sampling parameters cost: a same-box A/B of the lock-step
batch decode on the synthetic 1.7B model, 128 fixed frames, at batch 8 and 32:

  (a) unarmed                         the plain samplers (k_sample_w)
  (b) armed, every row the defaults   the per-slot fast-only family (k_sample_pw)
  (c) armed, mixed fast-path rows     the same family, rows differ
  (d) armed, one nucleus row          the general 256-thread kernel (k_sample_p)

and (a) once more on another build of the library (--parent-lib: the parent
commit's, `make VARIANT=_a` there), which must equal (a).  Every figure comes
from a fresh process (the variants alternate, --reps rounds); a process warms
up once and reports the median of 3 timed runs; the line per variant is the
median over the rounds.  audio-s/s = slots x frames x 0.08 s over the decode
loop's wall time (perf_talker_ms) and over the whole call (perf_total_ms).

  python tools/slot_params_ab.py [--parent-lib PATH] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, "qwen3-tts-c_amd")]

FRAMES = 128
BATCHES = (8, 32)
DEFAULT = dict(temperature=0.9, top_k=50, top_p=1.0, rep=1.05, st_temperature=0.9, st_top_k=50, st_top_p=1.0)
FAST_ROWS = [{}, dict(top_k=1, st_top_k=1), dict(rep=1.5), dict(top_k=300, st_top_k=7, temperature=0.6)]
NUCLEUS = dict(top_p=0.8, st_top_p=0.7)


def rows_of(variant, nb):
    if variant == "b":
        return [{} for _ in range(nb)]
    if variant == "c":
        return [dict(FAST_ROWS[b % 4], seed=42 + b) for b in range(nb)]
    if variant == "d":
        return [dict(NUCLEUS) if b == 0 else {} for b in range(nb)]
    return None


def child(variant):
    import qtts
    from synth_model import ensure_model, prompt_ids
    md = ensure_model(os.path.join(os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models"), "1.7b"), "1.7b", seed=0)
    m = qtts.QwenTTS(md)
    out = {"variant": variant, "lib": os.path.basename(os.path.dirname(qtts.LIB_PATH))}
    for nb in BATCHES:
        prompts = [prompt_ids("p128", seed=1234 + b) for b in range(nb)]
        m.set_params(max_tokens=4096, fixed=FRAMES, seed=42, **DEFAULT)
        talker, total = [], []
        n0 = qtts.Kernels.sample_slot_launches() if hasattr(qtts.Kernels, "sample_slot_launches") and \
            hasattr(qtts.lib(), "qtts_hip_sample_slot_launches") else None
        for run in range(4):   # one warm-up (graph capture, code objects), three timed
            rows = rows_of(variant, nb)
            if rows is not None:
                m.set_utterance_sampling(rows)
            rc, audio = m.generate_batch(prompts, ["aiden"] * nb, ["english"] * nb)
            assert rc == 0 and all(a is not None and len(a) == FRAMES * 1920 for a in audio)
            if run:
                talker.append(m.c.perf_talker_ms)
                total.append(m.c.perf_total_ms)
        if n0 is not None:   # the sampler that ran is the one the variant names
            assert (qtts.Kernels.sample_slot_launches() > n0) == (rows_of(variant, nb) is not None)
        sec = nb * FRAMES * 0.08
        out[f"b{nb}"] = {"decode_audio_s_per_s": round(sec / (statistics.median(talker) / 1e3), 1),
                         "total_audio_s_per_s": round(sec / (statistics.median(total) / 1e3), 1)}
    m.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    variants = [("a", None), ("b", None), ("c", None), ("d", None)]
    if a.parent_lib:
        variants.insert(0, ("a", a.parent_lib))
    got = {}
    for rep in range(a.reps):
        for v, libp in variants:
            env = dict(os.environ)
            env.pop("QTTS_LIB", None)
            if libp:
                env["QTTS_LIB"] = os.path.abspath(libp)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", v], env=env, capture_output=True,
                               text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"variant {v} ({libp or 'this build'}) failed")
            rec = json.loads(line[0][7:])
            print(f"round {rep} {'parent ' if libp else ''}({v}): {json.dumps(rec)}", flush=True)
            got.setdefault((v, bool(libp)), []).append(rec)
    names = {"a": "unarmed", "b": "armed, all rows default", "c": "armed, mixed fast-path rows",
             "d": "armed, one nucleus row (general kernel)"}
    lines = []
    for (v, parent), recs in got.items():
        for nb in BATCHES:
            dec = statistics.median(r[f"b{nb}"]["decode_audio_s_per_s"] for r in recs)
            tot = statistics.median(r[f"b{nb}"]["total_audio_s_per_s"] for r in recs)
            lines.append(f"batch {nb:2d} ({v}) {names[v]}{' [parent commit build]' if parent else ''}: "
                         f"decode {dec:.1f} audio-s/s, whole call {tot:.1f} audio-s/s "
                         f"(median of {len(recs)} processes; per process "
                         f"{[r[f'b{nb}']['decode_audio_s_per_s'] for r in recs]})")
    lines.sort()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/slot_params_ab.py: synthetic 1.7B, {FRAMES} fixed frames, alternating fresh processes\n")
            f.write(text)


if __name__ == "__main__":
    main()
