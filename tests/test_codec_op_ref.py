"""codec_op_ref.py's bars tell a right kernel from a wrong one, on a CPU box:
an fp32 numpy restatement of every small codec kernel passes every case of
codec_op_cases.py (bound class: with err / bound below 1, recorded in the
message), and each deliberate defect fails at least one case: the inputs make
every defect visible before anything runs on a device."""
import numpy as np
import pytest

import codec_op_cases as CS

ALL = CS.CASES + CS.TWINS


@pytest.mark.parametrize("c", ALL, ids=[c.id() for c in ALL])
def test_faithful_restatement_passes(c):
    ratio = c.check(c.run_model())
    assert ratio < 1.0, (c.id(), f"err / bound {ratio:.4f}")
    print(f"err / bound  {c.id():48s} {ratio:.4f}")
    if c.twin is not None:
        assert c.twin_same(c.run_model(), c.twin.run_model()), "the n = 1 launch differs from its single-plane twin"


def test_every_kernel_has_a_case():
    assert {c.kernel for c in ALL} == set(CS.KERNELS)


def test_untouched_output_fails():
    """a launch that writes nothing fails every case: no check is vacuous"""
    for c in ALL:
        outs = [np.array(o[0] if isinstance(o, tuple) else o) for o in c.out]
        with pytest.raises(AssertionError):
            c.check(outs)


def _killed(kernels, mut):
    killed = []
    for c in ALL:
        if c.kernel in kernels and mut in c.muts:
            try:
                c.check(c.run_model((mut,)))
            except AssertionError:
                killed.append(c.id())
    return killed


DEFECTS = [  # (what, kernels, the model's name for it)
    ("one-pass variance", ("k_ln_t", "k_ln_t_ms"), "one_pass"),
    ("eps dropped (LayerNorm)", ("k_ln_t", "k_ln_t_ms"), "no_eps"),
    ("eps dropped (RMSNorm)", ("k_rms_rows",), "no_eps"),
    ("biased by C - 1 (LayerNorm)", ("k_ln_t", "k_ln_t_ms"), "biased"),
    ("biased by D - 1 (RMSNorm)", ("k_rms_rows",), "biased"),
    ("RoPE upper-half index swapped", ("k_rope_rows",), "swap"),
    ("RoPE upper-half index swapped (ms)", ("k_rope_kv_ms",), "swap"),
    ("RoPE position off by one", ("k_rope_rows",), "pos"),
    ("RoPE position off by one (ms)", ("k_rope_kv_ms",), "pos"),
    ("RVQ projection without lanes >= vq - vq % 64", ("k_rvq_proj", "k_rvq_proj_ms"), "lanes"),
    ("RVQ projection with s1 only", ("k_rvq_proj", "k_rvq_proj_ms"), "s1_only"),
    ("dwconv with the first tap dropped", ("k_dwconv", "k_dwconv_ms"), "tap0"),
    ("dwconv reading the margin at tmin = 0", ("k_dwconv", "k_dwconv_ms"), "margin"),
    ("history save from L - H", ("k_hist_ms",), "from_L"),
    ("keep-shift by shift + 1", ("k_kv_shift_ms",), "plus"),
    ("keep-shift by shift - 1", ("k_kv_shift_ms",), "minus"),
    ("keep-shift computed from hl + T", ("k_kv_shift_ms",), "hl_T"),
    ("pad row storing K / V", ("k_rope_kv_ms",), "pad_store"),
    ("clamp writing L samples", ("k_clamp_ms",), "all"),
    ("sid ignored (history)", ("k_hist_ms",), "sid"),
    ("sid ignored (K / V rows)", ("k_rope_kv_ms",), "sid"),
    ("sid ignored (attention rows)", ("k_ms_index",), "sid"),
]


@pytest.mark.parametrize("what,kernels,mut", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_defect_fails_a_case(what, kernels, mut):
    killed = _killed(kernels, mut)
    print(f"{what}: {len(killed)} cases fail, e.g. {killed[:2]}")
    assert killed, what
    for k in kernels:                       # each twin on its own, not only the family
        assert any(i.startswith(k + "-") for i in killed), (what, k)
