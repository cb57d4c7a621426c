#!/usr/bin/env python3
"""The arguments of every launch of a decode frame and of a prefill, on two
builds of the library: line for line the same, and the same codes out.

Both libraries are built with `make EXTRA=-DQTTS_ARGDUMP` (csrc/hip/qtts_argdump.h):
every launcher entry then appends one text line per call -- its scalar
arguments and its pointers as p<k> in order of first appearance -- to the file
QTTS_ARGDUMP_FILE names.  A kernel trace cannot see prefetch slices, partial
pointers or strides; this dump does.  Graph capture issues every launch once,
so a case needs only a prompt, the prefill and three frames.

Every case and side is a fresh child process (QTTS_LIB selects its library,
the case's environment switches are set for it alone); the dump covers the
child from the model load on, so the load-time table builders are in every
case.  Memory copies, memsets and allocations are not launcher entries and are
not in the dump.

  python tools/frame_args_ab.py --parent-lib PATH --lib PATH [--out FILE] [--work DIR] [--only SUBSTR] [--jobs N]

--parent-lib / --lib: the parent commit's and this tree's dump builds (`make
VARIANT=_x EXTRA=-DQTTS_ARGDUMP`; the hooks and the header apply unchanged to
the parent).
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, "qwen3-tts-c_amd")]

SPK, LANG = "aiden", "english"
WIDE = dict(Hs=1024, Is=1024, HDs=128)            # sub-talker shapes of the lean kernels (the pair pass runs)
WIDE_EQ = dict(H=1024, Hs=1024, Is=1024, HDs=128)


def _cases():
    """name -> (kind, model, overrides, batch, environment)"""
    c = {}
    b1 = [{}, {"QTTS_HIP_ST_PAIR": "0"}, {"QTTS_HIP_ATTN_O": "0"}, {"QTTS_HIP_PTAB": "0"}, {"QTTS_HIP_L2PF": "0"},
          {"QTTS_HIP_ATTN_DEFER": "0"}, {"QTTS_HIP_NO_GRAPH": "1"}]
    tag = lambda env: "_".join(f"{k[9:].lower()}{v}" for k, v in env.items()) or "default"
    for model, over in (("tiny", {}), ("tiny_eq", {}), ("tiny", WIDE)):
        for env in b1:
            c[f"{model}{'_wide' if over else ''}_b1_{tag(env)}"] = ("gen", model, over, 1, env)
    c["tiny_eq_wide_b1_default"] = ("gen", "tiny_eq", WIDE_EQ, 1, {})
    for nb in (2, 8, 9, 16, 17, 64):
        c[f"tiny_b{nb}_default"] = ("gen", "tiny", {}, nb, {})
    for env in ({"QTTS_HIP_TAB0B": "0"}, {"QTTS_HIP_BSPLIT": "0"}, {"QTTS_HIP_GEMVB": "0"}, {"QTTS_HIP_BSELF_MIN": "2"},
                {"QTTS_HIP_BKZ_MAX": "4"}, {"QTTS_HIP_BKZ_WIDE": "0"}, {"QTTS_HIP_BKZ_WIDE": "2"}):
        c[f"tiny_b8_{tag(env)}"] = ("gen", "tiny", {}, 8, env)
    c["tiny_wide_b8_default"] = ("gen", "tiny", WIDE, 8, {})
    c["tiny_wide_b8_tab0b0"] = ("gen", "tiny", WIDE, 8, {"QTTS_HIP_TAB0B": "0"})
    for nb in (1, 8, 16, 32):
        c[f"1.7b_b{nb}_default"] = ("gen", "1.7b", {}, nb, {})
    c["1.7b_b1_l2pf_tk3"] = ("gen", "1.7b", {}, 1, {"QTTS_HIP_L2PF_TK": "3"})
    c["1.7b_b1_kv_bf16"] = ("gen", "1.7b", {}, 1, {"QTTS_HIP_KV": "bf16"})
    c["1.7b_b8_kv_bf16"] = ("gen", "1.7b", {}, 8, {"QTTS_HIP_KV": "bf16"})
    c["0.6b_b1_default"] = ("gen", "0.6b", {}, 1, {})
    for pg in ({}, {"QTTS_HIP_PGEMM": "0"}):
        t = "_pgemm0" if pg else ""
        c["prefill_custom_voice" + t] = ("gen_short", "1.7b", {}, 1, pg)      # <= 16 prompt rows
        c["prefill_p128" + t] = ("gen", "1.7b", {}, 1, pg)
        c["prefill_vc_80" + t] = ("vc", "1.7b", {}, 1, pg)                    # > 64 rows
        c["prefill_vc_b8" + t] = ("vc", "tiny", {}, 8, pg)
    c["queue_refill_instruct"] = ("queue", "tiny", {}, 3, {})
    c["fed"] = ("fed", "tiny", {}, 1, {})
    c["forced"] = ("forced", "tiny", {}, 1, {})
    c["slot_params_nucleus"] = ("slots", "tiny", {}, 2, {})
    c["stage_entries"] = ("stages", "tiny", {}, 1, {})
    c["load_tiny"] = ("load", "tiny", {}, 1, {})
    c["load_1.7b"] = ("load", "1.7b", {}, 1, {})
    return c


CASES = _cases()


def model_dir(model, over):
    from synth_model import ensure_model
    root = os.environ.get("QTTS_TEST_MODELS", "/tmp/qtts_test_models")
    tag = model + "".join(f"_{k}{v}" for k, v in sorted(over.items()))
    return ensure_model(os.path.join(root, tag), model, seed=0, overrides=over or None)


def child(name, out_path):
    import numpy as np
    import qtts
    from synth_model import prompt_ids
    kind, model, over, nb, _ = CASES[name]
    m = qtts.QwenTTS(model_dir(model, over))
    rng = np.random.default_rng(7)
    m.set_params(max_tokens=8, fixed=3, seed=42)
    prompts = [prompt_ids("p128", 1300 + b) for b in range(nb)]
    codes = []
    if kind == "load":
        pass
    elif kind in ("gen", "gen_short"):
        if kind == "gen_short":
            prompts = [prompt_ids("short")]
        if nb == 1:
            assert m.generate(prompts[0], SPK, LANG) is not None
            codes = [m.last_codes()]
        else:
            rc, _ = m.generate_batch(prompts, [SPK] * nb, [LANG] * nb)
            assert rc == 0, rc
            codes = [m.last_codes_slot(b, 3) for b in range(nb)]
    elif kind == "vc":
        ref_ids = [151644, 77091, 198, 2354, 2244, 151645, 198]
        ref = [rng.integers(0, 2048, size=(80 if nb == 1 else 20 + b, 16)).astype(np.int32) for b in range(nb)]
        spk = [(rng.standard_normal(m.cfg.talker_hidden) * 0.1).astype(np.float32) for _ in range(nb)]
        if nb == 1:
            assert m.generate_voice_clone(prompts[0], ref_ids, ref[0], spk[0], LANG) is not None
            codes = [m.last_codes()]
        else:
            rc, _ = m.generate_voice_clone_batch(prompts, [ref_ids] * nb, ref, spk, [LANG] * nb)
            assert rc == 0, rc
            codes = [m.last_codes_slot(b, 3) for b in range(nb)]
    elif kind == "queue":   # 5 utterances on 3 slots: a refill; instruct prefix A misses, then hits, B misses
        prompts = [prompt_ids("p128", 1300 + b) for b in range(5)]
        ia, ib = rng.integers(1000, 100000, size=12).tolist(), rng.integers(1000, 100000, size=7).tolist()
        m.set_utterance_instruct([ia, None, ia, ib, ia])
        rc, _ = m.generate_queue(prompts, [SPK] * 5, [LANG] * 5, slots=3)
        assert rc == 0, rc
        codes = [m.queue_codes(i) for i in range(5)]
    elif kind == "fed":
        ids, sent = list(prompts[0][3:-5]), []

        def feed(h, wait):
            if not sent:
                assert h.push(0, ids) == 0 and h.close(0) == 0
                sent.append(1)
        assert m.generate_fed_stream(feed, SPK, LANG, chunk_frames=4) is not None
        codes = [m.last_codes_slot(0, 3)]
    elif kind == "forced":
        m.force_codes(rng.integers(0, 2048, size=(2, 16)).astype(np.int32))
        assert m.generate(prompts[0], SPK, LANG) is not None
        codes = [m.last_codes()]
    elif kind == "slots":   # row 1 draws from a nucleus: the general per-slot sampler's graphs
        m.set_utterance_sampling([{"seed": 5}, {"seed": 6, "top_p": 0.8, "top_k": 0}])
        rc, _ = m.generate_batch(prompts, [SPK] * nb, [LANG] * nb)
        assert rc == 0, rc
        codes = [m.last_codes_slot(b, 3) for b in range(nb)]
    elif kind == "stages":
        H = m.cfg.talker_hidden
        hid = m.prefill((rng.standard_normal((12, H)) * 0.5).astype(np.float32))
        step = m.step((rng.standard_normal(H) * 0.5).astype(np.float32))
        sub = m.subtalker((rng.standard_normal(H) * 0.5).astype(np.float32), 5)
        codes = [np.asarray(x).ravel().view(np.int32) for x in (hid, *(step if isinstance(step, tuple) else (step,)), sub)]
    m.close()
    with open(out_path, "wb") as f:
        for c in codes:
            f.write(np.ascontiguousarray(c).tobytes())
    print("DONE", name, flush=True)


FAILED = []   # a child failed: no further child is started


def run_child(name, lib, work, side):
    if FAILED:
        raise SystemExit(f"case {name} not run: {FAILED[0]} failed")
    d = os.path.join(work, side)
    os.makedirs(d, exist_ok=True)
    dump, codes = os.path.join(d, name + ".dump"), os.path.join(d, name + ".codes")
    for p in (dump, codes):
        if os.path.exists(p):
            os.remove(p)
    env = dict(os.environ, QTTS_LIB=os.path.abspath(lib), QTTS_ARGDUMP_FILE=dump, **CASES[name][4])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--codes", codes], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 or "DONE " + name not in r.stdout:
        FAILED.append(name)
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"case {name} on {lib} failed ({r.returncode})")
    with open(dump) as f:
        lines = f.read().splitlines()
    with open(codes, "rb") as f:
        return lines, f.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--codes")
    ap.add_argument("--parent-lib")
    ap.add_argument("--lib")
    ap.add_argument("--only", default="")
    ap.add_argument("--jobs", type=int, default=4, help="child processes at a time")
    ap.add_argument("--work", default=os.path.join(ROOT, "ab_out", "frame_args"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.codes)
    if not a.parent_lib or not a.lib:
        raise SystemExit("--parent-lib PATH and --lib PATH (both built with EXTRA=-DQTTS_ARGDUMP) are required")
    out, bad = [f"# tools/frame_args_ab.py: parent library {a.parent_lib} against {a.lib}",
                "# case, dump lines parent / this build, code bytes, verdict"], 0
    from concurrent.futures import ThreadPoolExecutor
    names = [n for n in CASES if a.only in n]
    for n in names:   # (the synthetic models are written here, once, not by children side by side)
        model_dir(CASES[n][1], CASES[n][2])
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:   # (each job is a child process of its own)
        jobs = {(n, side): ex.submit(run_child, n, lib, a.work, side)
                for n in names for side, lib in (("parent", a.parent_lib), ("branch", a.lib))}
        res = {k: f.result() for k, f in jobs.items()}
    for name in names:
        (lp, cp), (lb, cb) = res[name, "parent"], res[name, "branch"]
        same = lp == lb and cp == cb and (len(lp) > 0)
        line = f"{name:34s} {len(lp):6d} / {len(lb):6d} lines  {len(cb):6d} code bytes  "
        line += "identical, codes equal" if same else "DIFFERENT"
        if lp != lb:
            k = next((i for i, (x, y) in enumerate(zip(lp, lb)) if x != y), min(len(lp), len(lb)))
            line += f"\n    first at line {k}:\n    parent: {lp[k] if k < len(lp) else None}\n    branch: {lb[k] if k < len(lb) else None}"
        elif cp != cb:
            line += " (codes)"
        bad += not same
        out.append(line)
        print(line, flush=True)
    out.append("verdict: " + ("every case has identical dumps and equal codes" if not bad else f"{bad} case(s) differ"))
    print(out[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
