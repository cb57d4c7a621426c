#!/usr/bin/env python3
"""Every draw of a reference fixture under the reference's own history, and a
two-sided verdict on each one that differs (tests/forced.py).

  python tools/classify_forced.py --fixture long_hd128_max [--write]

1. GPU: the fixture's utterance with the reference's codes forced
   (QwenTTS.force_codes); every draw where the free-draw record differs from
   the reference is collected.
2. GPU: the same run again with logit taps on those draws, at most 8 per run.
3. CPU: the oracle port replays the utterance to each draw
   (Oracle.trace_draw) and tests/forced.py classify_two_sided gives the
   verdict: the reference's draw within rounding of a decision boundary AND
   the GPU's logits within CARRY x the head GEMV's rounding bound of the
   reference's.

--write merges the result into tests/golden/forced_near_ties.json (recorded
results only: fixture, frame, group, reference id, drawn id, eps_flip,
eps_gemv, the GPU-side max logit error, both ratios, verdict).
--taps-out FILE stops after step 2 and keeps the taps (npz); --taps-in FILE
starts at step 3 from such a file, on a machine without the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "qwen3-tts-c_amd")]
from conftest import model_dir  # noqa: E402
from forced import classify_two_sided  # noqa: E402
from oracle_py import DEFAULT, Oracle  # noqa: E402
from qtts_io import lookup_ids  # noqa: E402

# fixture -> (long_manifest.json key, model preset, codes array)
KEYS = {"long_hd128_max": ("hd128max", "hd128", "codes"), "long_hd128": ("hd128", "hd128", "decode_codes")}
OUT = os.path.join(ROOT, "tests", "golden", "forced_near_ties.json")
MAX_TAPS = 8


def load(fixture):
    key, preset, ck = KEYS[fixture]
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture + ".npz"))
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "long_manifest.json")))[key]
    # the fixed-length runs of tests/test_gpu_long.py
    mx = man["frames"] if key == "hd128max" else 4096
    return dict(ids=g["prompt_ids"], ref=g[ck], preset=preset, speaker=man.get("speaker", "aiden"),
                language=man.get("language", "english"),
                params=dict(max_tokens=mx, fixed=man["frames"], seed=man["seed"], **DEFAULT))


def gpu_phase(fx):
    import qtts
    m = qtts.QwenTTS(model_dir(fx["preset"]))
    try:
        def run(taps):
            m.set_params(**fx["params"])
            m.force_codes(fx["ref"])
            for f, g in taps:
                m.tap_draw(f, g)
            assert m.generate(fx["ids"], fx["speaker"], fx["language"]) is not None
            assert np.array_equal(m.last_codes(), fx["ref"]), "the stored codes are not the forced ones"
            return m.last_drawn()
        d = run([])
        assert d.shape == fx["ref"].shape, (d.shape, fx["ref"].shape)
        bad = [(int(f), int(g)) for f, g in np.argwhere(d != fx["ref"])]
        print(f"{d.size} draws, {len(bad)} differ from the reference: {[(f, g, int(d[f, g])) for f, g in bad]}")
        taps = {}
        for i in range(0, len(bad), MAX_TAPS):
            chunk = bad[i:i + MAX_TAPS]
            d2 = run(chunk)
            assert np.array_equal(d2, d), "the free-draw record is not reproducible"
            for j, fg in enumerate(chunk):
                lg, bits, drawn = m.tap_result(j)
                assert drawn == d[fg], (fg, drawn, int(d[fg]))
                taps[fg] = (lg, bits, drawn)
        return bad, taps
    finally:
        m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="long_hd128_max", choices=sorted(KEYS))
    ap.add_argument("--write", action="store_true", help="merge into tests/golden/forced_near_ties.json")
    ap.add_argument("--taps-out", default=None)
    ap.add_argument("--taps-in", default=None)
    a = ap.parse_args()
    fx = load(a.fixture)
    if a.taps_in:
        z = np.load(a.taps_in)
        bad = [tuple(int(v) for v in fg) for fg in z["draws"]]
        taps = {fg: (z[f"lg{i}"], int(z["bits"][i]), int(z["drawn"][i])) for i, fg in enumerate(bad)}
    else:
        bad, taps = gpu_phase(fx)
        if a.taps_out:
            np.savez(a.taps_out, draws=np.array(bad, np.int64).reshape(-1, 2),
                     bits=np.array([taps[fg][1] for fg in bad], np.uint32),
                     drawn=np.array([taps[fg][2] for fg in bad], np.int32),
                     **{f"lg{i}": taps[fg][0] for i, fg in enumerate(bad)})
            print(f"taps of {len(bad)} draws -> {a.taps_out}")
            return
    o = Oracle(model_dir(fx["preset"]))
    s, l = lookup_ids(o.cfg, fx["speaker"], fx["language"])
    rows = []
    for f, g in bad:
        c = classify_two_sided(o, taps[(f, g)], fx["ids"], s, l, f, g, fx["params"])
        assert c.get("reference") in (None, int(fx["ref"][f, g])), ("the oracle's draw is not the fixture's", c)
        row = dict(fixture=a.fixture, frame=f, group=g, reference=int(fx["ref"][f, g]), drawn=int(taps[(f, g)][2]))
        row.update({k: c[k] for k in ("eps_flip", "eps_gemv", "gpu_err", "ratio_ref", "ratio_gpu", "verdict_ref",
                                      "verdict") if k in c})
        if "why" in c:
            row["why"] = c["why"]
        rows.append(row)
        print(json.dumps(row))
    o.close()
    if a.write:
        doc = json.load(open(OUT)) if os.path.exists(OUT) else {"generator": "tools/classify_forced.py", "draws": []}
        doc["draws"] = [r for r in doc["draws"] if r["fixture"] != a.fixture] + rows
        with open(OUT, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        print(f"{len(rows)} draws of {a.fixture} -> {OUT}")


if __name__ == "__main__":
    main()
