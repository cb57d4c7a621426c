#!/usr/bin/env python3
"""What top_p < 1 costs with the nucleus short list (k_sample_n.hip): a
same-box A/B on the synthetic 1.7B model, 128 fixed frames.

  batch 8 and 32 (lock-step generate_batch):
    (b) armed, every row the defaults            the per-slot fast-only family
    (d) armed, one nucleus row (0.8 / 0.7)       the general per-slot kernel
    (n) unarmed, ctx-wide top_p 0.8 / 0.7        the plain kernel
  batch 1 (generate):
    (a) the defaults    (n) ctx-wide top_p 0.8 / 0.7

on three builds / settings, alternating, each in a fresh process per round:
this build, this build with QTTS_HIP_SAMPLE_NUCLEUS=0 (the in-build control:
the full-path kernels of before) and, with --parent-lib, the parent commit's
library (`make VARIANT=_a` there).  A process warms every variant up once and
reports the median of 3 timed runs; the table holds the median over the rounds.
audio-s/s = slots x frames x 0.08 s over the decode loop's wall time
(perf_talker_ms).

  python tools/nucleus_ab.py [--parent-lib PATH] [--reps 3] [--out FILE]
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
NUCLEUS = dict(top_p=0.8, st_top_p=0.7)
NAMES = {"a": "defaults", "b": "armed, all rows default", "d": "armed, one nucleus row",
         "n": "ctx-wide top_p 0.8 / 0.7"}


def child():
    import qtts
    from synth_model import ensure_model, prompt_ids
    md = ensure_model(os.path.join(os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models"), "1.7b"), "1.7b", seed=0)
    m = qtts.QwenTTS(md)
    out = {}

    def timed(run):
        t = []
        for i in range(4):   # one warm-up (graph capture, code objects), three timed
            run()
            if i:
                t.append(m.c.perf_talker_ms)
        return statistics.median(t)

    for nb in BATCHES:
        prompts = [prompt_ids("p128", seed=1234 + b) for b in range(nb)]
        for v in ("b", "d", "n"):
            def run():
                m.set_params(max_tokens=4096, fixed=FRAMES, seed=42, **dict(DEFAULT, **(NUCLEUS if v == "n" else {})))
                if v != "n":
                    m.set_utterance_sampling([dict(NUCLEUS) if v == "d" and b == 0 else {} for b in range(nb)])
                rc, audio = m.generate_batch(prompts, ["aiden"] * nb, ["english"] * nb)
                assert rc == 0 and all(a is not None and len(a) == FRAMES * 1920 for a in audio)
            out[f"b{nb}{v}"] = round(nb * FRAMES * 0.08 / (timed(run) / 1e3), 1)
    ids = prompt_ids("p128", seed=1234)
    for v in ("a", "n"):
        def run():
            m.set_params(max_tokens=4096, fixed=FRAMES, seed=42, **dict(DEFAULT, **(NUCLEUS if v == "n" else {})))
            a = m.generate(ids, "aiden", "english")
            assert a is not None and len(a) == FRAMES * 1920
        out[f"b1{v}"] = round(FRAMES * 0.08 / (timed(run) / 1e3), 2)
    m.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child()
    builds = [("this build", None, None), ("this build, QTTS_HIP_SAMPLE_NUCLEUS=0", None, "0")]
    if a.parent_lib:
        builds.insert(0, ("parent commit build", a.parent_lib, None))
    got = {}
    for rep in range(a.reps):
        for name, libp, sw in builds:
            env = dict(os.environ)
            env.pop("QTTS_LIB", None)
            env.pop("QTTS_HIP_SAMPLE_NUCLEUS", None)
            if libp:
                env["QTTS_LIB"] = os.path.abspath(libp)
            if sw is not None:
                env["QTTS_HIP_SAMPLE_NUCLEUS"] = sw
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                               text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{name} failed")
            rec = json.loads(line[0][7:])
            print(f"round {rep} {name}: {json.dumps(rec)}", flush=True)
            got.setdefault(name, []).append(rec)
    lines = []
    for key in [f"b{nb}{v}" for nb in BATCHES for v in ("b", "d", "n")] + ["b1a", "b1n"]:
        nb, v = int(key[1:-1]), key[-1]
        for name, _, _ in builds:
            per = [r[key] for r in got[name]]
            lines.append(f"batch {nb:2d} ({v}) {NAMES[v]} [{name}]: decode {statistics.median(per)} audio-s/s "
                         f"(median of {len(per)} processes; per process {per})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# tools/nucleus_ab.py: synthetic 1.7B, {FRAMES} fixed frames, alternating fresh processes\n")
            f.write(text)


if __name__ == "__main__":
    main()
