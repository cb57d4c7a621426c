"""Every small kernel of the codec decoder (k_codec.hip: the kernels between
the contractions and the multi-stream placement kernels) on the device through
qtts_hip_codec_op, which launches each through the helper the network uses,
against the references and bounds of codec_op_ref.py on the cases of
codec_op_cases.py: outputs finite where defined, within the bound or bit-equal
by class, sentinels and inputs bit-identical after the launch, and every
multi-stream kernel at n = 1 bit-equal to its single-plane twin.
test_codec_op_ref.py checks on the same inputs that the bars would notice a
wrong kernel."""
import numpy as np
import pytest

import codec_op_cases as CS
import qtts
from codec_op_ref import same

pytestmark = pytest.mark.gpu

_RATIO = {}


def _note(name, ratio):
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    print(f"err / bound  {name:24s} {ratio:.4f}")


def _launch(c, gpu):
    """uploads the case, launches, returns the outputs after; asserts the inputs unchanged"""
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    outs = [dev(o[0] if isinstance(o, tuple) else o) for o in c.out]
    ooff = [o[1] if isinstance(o, tuple) else 0 for o in c.out]
    held, args = [], []
    for a in c.inp:
        if a is None:
            args.append(None)
        elif isinstance(a, tuple) and isinstance(a[0], str):      # ("ptrs", ...)
            t = dev(np.array([outs[j].data_ptr() + 4 * off for j, off in a[1]], np.int64))
            held.append((t, t.cpu().numpy()))
            args.append(t)
        else:
            arr, off = a if isinstance(a, tuple) else (a, 0)
            t = dev(arr)
            held.append((t, np.ascontiguousarray(arr)))
            args.append(t.data_ptr() + off * arr.itemsize)
    nout = c.meta.get("nout", len(outs))
    optr = [outs[j].data_ptr() + ooff[j] * outs[j].element_size() for j in range(nout)]
    assert qtts.Kernels.codec_op(c.op, args, optr, c.n, c.s, c.eps), c.id()
    torch.cuda.synchronize()
    for t, before in held:
        assert same(t.cpu().numpy(), before), (c.id(), "the launch wrote to an input")
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("c", CS.CASES, ids=[c.id() for c in CS.CASES])
def test_codec_op(gpu, c):
    _note(c.kernel, c.check(_launch(c, gpu)))


@pytest.mark.parametrize("c", CS.TWINS, ids=[c.id() for c in CS.TWINS])
def test_one_stream_equals_the_single_plane_kernel(gpu, c):
    mine = _launch(c, gpu)
    _note(c.kernel, c.check(mine))
    assert c.twin_same(mine, _launch(c.twin, gpu)), (c.id(), c.twin.id())


def test_refusals_on_the_device(gpu):
    """what the launch helpers refuse comes back False and launches nothing"""
    import torch
    x = torch.zeros(64, device=gpu)
    i = torch.zeros(64, dtype=torch.int32, device=gpu)
    assert not qtts.Kernels.codec_op(qtts.CO_RVQ_SUM, (i, x), (x, x), (1, 1, 4, 1025))       # vq > 1024
    assert not qtts.Kernels.codec_op(qtts.CO_ROPE_ROWS, (x, x), (x,), (1, 30, 2, 15))         # odd hd
    assert not qtts.Kernels.codec_op(99, (), (), ())
    torch.cuda.synchronize()
    assert not x.any()


def test_zz_ratios(gpu):
    """prints the largest err / bound per kernel seen above (for codec_op_ref.MEASURED)"""
    for k in sorted(_RATIO):
        print(f"err / bound  {k:32s} {_RATIO[k]:.4f}")
