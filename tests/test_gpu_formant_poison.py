"""GPU: taco_frames_formant on a POISONED output between guard bands (tests/poison.py), in the style of tests/test_gpu_poison.py: the
contract hands the call an `out` with arbitrary contents and promises that every element of it is written and nothing outside it.
Each case runs once on an output of zeros and then on outputs filled with `qnan`, `ones` and `noise`, with the same poison in the
columns of mag_t behind every row's end.  Asserted: the output is BIT-identical to the clean run, no element still holds poison,
the guard bands around mag_t and out are bytewise intact, and mag_t is unwritten.  Nothing here makes a kernel misbehave: the poison
goes only where the contract allows arbitrary contents."""
import numpy as np
import pytest
import torch

from tests import formant_ref as fr
from tests import poison
from tests.poison import Guarded

pytestmark = pytest.mark.gpu

GUARD_FLOATS = 4096          # 16 KiB of sentinel around every buffer: a whole 32-frame tile row of overrun lands inside it
CASES = {c[0]: c[1:] for c in fr.all_cases()}
NAMES = ('mixed_C129_Q32_F33', 'mixed_C129_Q64_F65', 'mixed_C17_Q8_F31', 'beside_one', 'per_unit_3', 'production')


def call(lib, x, frames, steps, Q, per_unit, fill, shift=0):
    """the call with `out` (and the columns of mag_t behind each row's end) holding `fill` -> out's bits on the host"""
    B, Cw, F = x.shape
    G = Guarded({'in': ((x.size + shift,), torch.float32, 'zeros'), 'out': ((x.size + shift,), torch.float32, fill)}, guard_floats=GUARD_FLOATS)
    xin, out = G['in'][shift:].view(B, Cw, F), G['out'][shift:].view(B, Cw, F)
    src = torch.from_numpy(x).cuda()
    if fill != 'zeros':   # behind a row's end mag_t may hold anything: the poison of the output
        junk = torch.empty(x.size, dtype=torch.float32, device='cuda')
        poison.poison(junk, fill, seed=5)
        junk = junk.view(B, Cw, F)
        for b in range(B):
            Fb = fr.row_frames(None if frames is None else frames[b], per_unit, F)
            src[b, :, Fb:] = junk[b, :, Fb:]
    xin.copy_(src)
    before = xin.clone()
    lib.frames_formant(xin, None if frames is None else torch.tensor(frames, dtype=torch.int32).cuda(),
                       torch.tensor(steps, dtype=torch.int32).cuda(), per_unit, Q, out=out)
    torch.cuda.synchronize()
    G.check()
    assert bool(poison.untouched(G['out'][:shift], G.marks['out']).all()), 'the floats in front of out were written'
    assert torch.equal(xin.view(torch.int32), before.view(torch.int32)), 'mag_t was written'
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('name', NAMES)
def test_poisoned_output_between_guard_bands(built_lib, name):
    x, frames, r, steps, Q = CASES[name]
    clean = call(built_lib, x, frames, steps, Q, r, 'zeros')
    want = fr.formant(x, frames, steps, r, Q)
    assert fr.rel_err(clean.view(np.float32), want) <= fr.FORMANT_RTOL
    for fill in poison.PATTERNS:
        for shift in (0, 1):
            got = call(built_lib, x, frames, steps, Q, r, fill, shift)
            assert np.isfinite(got.view(np.float32)).all(), '%s: an element of out still holds poison' % fill
            assert np.array_equal(got, clean), '%s, out %d floats behind its boundary: the bits depend on what out or the columns ' \
                                               'behind a row held' % (fill, shift)
