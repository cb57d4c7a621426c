"""The launch list of a decode frame: what qtts_dev_profile_frame reports for
step 0 (no talker) and step 1 (talker first) after a two-frame generate, as
the ordered list of [kind, kernel name, bytes] -- no timing.

tests/golden/frame_launches.json holds the lists of the cases below, recorded
once (python tests/frame_launches.py --record) from the build its "header"
entry names; tests/test_gpu_frame_launches.py and tests/test_gpu_full.py
require today's lists to equal them.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "frame_launches.json")

# the sub-talker shapes k_gemvw takes (tests/test_gpu_st_pair.py): with them the
# pair pass, the fused attention + O and the layer-0 table run at batch 1
WIDE = dict(Hs=1024, Is=1024, HDs=128)
WIDE_EQ = dict(H=1024, Hs=1024, Is=1024, HDs=128)

# name: (preset, model overrides, batch, environment)
CASES = {
    "tiny_b1": ("tiny", {}, 1, {}),
    "tiny_b1_st_pair0": ("tiny", {}, 1, {"QTTS_HIP_ST_PAIR": "0"}),
    "tiny_b1_attn_o0": ("tiny", {}, 1, {"QTTS_HIP_ATTN_O": "0"}),
    "tiny_b2": ("tiny", {}, 2, {}),
    "tiny_b17": ("tiny", {}, 17, {}),
    "tiny_eq_b1": ("tiny_eq", {}, 1, {}),
    "tiny_wide_b1": ("tiny", WIDE, 1, {}),
    "tiny_wide_b1_st_pair0": ("tiny", WIDE, 1, {"QTTS_HIP_ST_PAIR": "0"}),
    "tiny_wide_b1_attn_o0": ("tiny", WIDE, 1, {"QTTS_HIP_ATTN_O": "0"}),
    "tiny_wide_b2": ("tiny", WIDE, 2, {}),
    "tiny_wide_b17": ("tiny", WIDE, 17, {}),
    "tiny_eq_wide_b1": ("tiny_eq", WIDE_EQ, 1, {}),
}
FULL_CASE = "full_1.7b_b1"   # tests/test_gpu_full.py, on its own model


def frame_launches(m, nb):
    """two frames at batch nb on the loaded model m, then the launch lists of
    an eager step 0 and step 1: {"step0": [[kind, name, bytes], ...], "step1": ...}"""
    import qtts
    from synth_model import prompt_ids
    L = qtts.lib()
    L.qtts_dev_profile_frame.restype = C.c_int
    L.qtts_dev_profile_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ids = prompt_ids("short")
    m.set_params(max_tokens=8, fixed=2, seed=42)

    def run(n):
        if n == 1:
            assert m.generate(ids, "aiden", "english") is not None
        else:
            rc, _ = m.generate_batch([ids] * n, ["aiden"] * n, ["english"] * n)
            assert rc == 0, rc
    # A run at another slot count first: the run that counts then allocates the state anew, at exactly
    # its own capacity.  A context that other tests used keeps the largest capacity it was given, and
    # the talker's O projection picks its kernel by the attention splits of that capacity.
    run(2 if nb == 1 else 1)
    run(nb)
    out, n_max = {}, 4096
    for step in (0, 1):
        kind, byt, ms = (C.c_int * n_max)(), (C.c_double * n_max)(), (C.c_float * n_max)()
        names = C.create_string_buffer(n_max * 64)
        n = L.qtts_dev_profile_frame(m.c.hip, step, n_max, kind, byt, ms, names)
        assert 0 < n <= n_max, n
        out[f"step{step}"] = [[int(kind[i]), names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode(), float(byt[i])]
                              for i in range(n)]
    return out


def case_launches(name):
    """loads the case's model under its environment and returns its launch lists"""
    import qtts
    from conftest import model_dir
    preset, over, nb, env = CASES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)   # (the switches are read when the context is created)
    try:
        m = qtts.QwenTTS(model_dir(preset, **over))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        return frame_launches(m, nb)
    finally:
        m.close()


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def first_difference(got, want):
    """None if the two launch lists are equal, else a line that names the first difference"""
    for step in ("step0", "step1"):
        g, w = got[step], want[step]
        for i, (x, y) in enumerate(zip(g, w)):
            if x != y:
                return f"{step} launch {i}: {x} here, {y} in the fixture"
        if len(g) != len(w):
            return f"{step}: {len(g)} launches here, {len(w)} in the fixture"
    return None


def main():
    """--record BUILD: writes the fixture from the library in use (QTTS_LIB or the in-tree build)"""
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        raise SystemExit("usage: python tests/frame_launches.py --record 'BUILD (commit hash)'")
    sys.path[:0] = [HERE]
    import conftest  # noqa: F401  (puts the package and the tools on sys.path)
    import qtts
    out = {"header": {"recorded_from": sys.argv[2],
                      "what": "ordered [kind, kernel name, bytes] of qtts_dev_profile_frame, step 0 and step 1"}}
    for name in CASES:
        out[name] = case_launches(name)
        print(name, len(out[name]["step0"]), len(out[name]["step1"]), flush=True)
    m = qtts.QwenTTS(conftest.model_dir("1.7b"))
    out[FULL_CASE] = frame_launches(m, 1)
    m.close()
    print(FULL_CASE, len(out[FULL_CASE]["step0"]), len(out[FULL_CASE]["step1"]), flush=True)
    dst = os.environ.get("FRAME_LAUNCHES_OUT", FIXTURE)
    with open(dst, "w") as f:
        f.write("{\n" + ",\n".join(
            f' {json.dumps(k)}: ' + (json.dumps(v) if k == "header" else "{" + ", ".join(
                f'{json.dumps(s)}: [\n  ' + ",\n  ".join(json.dumps(e) for e in v[s]) + "]" for s in ("step0", "step1")) + "}")
            for k, v in out.items()) + "\n}\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
