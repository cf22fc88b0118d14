"""CPU checks of inference end detection: the NumPy restatement of the rule (tests/stop_ref.py) on hand-made alignments, and
the C ABI declaration (include/taco_hip.h) with its version."""
import os
import re

import numpy as np

from tests.stop_ref import stop_lengths

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')


def one_hot_path(path, Tt):
    """alignments (1, len(path), Tt) whose argmax at step t is path[t]"""
    al = np.full((1, len(path), Tt), 0.01, dtype=np.float32)
    for t, s in enumerate(path):
        al[0, t, s] = 0.9
    return al


def test_hold_across_a_block_boundary():
    # L = 6, end_offset 0: target 5.  The run starts at t = 2 and reaches hold 3 at t = 4, inside the second 4-step block
    al = one_hot_path([0, 3, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5], 8)
    assert stop_lengths(al, [6], 0, 3, 1)[0] == 8
    # an interruption restarts the run: 5, 5, (4), 5, 5, 5 -> t* = 7 -> len 8
    al = one_hot_path([0, 5, 5, 4, 5, 5, 5, 0, 0, 0, 0, 0], 8)
    assert stop_lengths(al, [6], 0, 3, 1)[0] == 8
    al = one_hot_path([0, 5, 5, 4, 5, 5, 0, 5, 5, 5, 0, 0], 8)
    assert stop_lengths(al, [6], 0, 3, 1)[0] == 12
    # positions past the target count: a_t >= target
    al = one_hot_path([7, 7, 0, 0], 8)
    assert stop_lengths(al, [6], 0, 2, 1)[0] == 4


def test_end_offset_at_or_past_the_text_length():
    # target 0: every step counts, so t* = max(hold, min_steps) - 1
    al = one_hot_path([0] * 20, 10)
    for L, off in ((5, 4), (5, 5), (5, 100), (1, 0)):
        assert stop_lengths(al, [L], off, 1, 1)[0] == 4
        assert stop_lengths(al, [L], off, 6, 1)[0] == 8
        assert stop_lengths(al, [L], off, 2, 9)[0] == 12
    # text_length is clamped to 1..Tt
    assert stop_lengths(al, [0], 0, 1, 1)[0] == 4
    assert stop_lengths(one_hot_path([9] * 8, 10), [50], 0, 1, 1)[0] == 4


def test_fire_on_the_last_step_and_never():
    al = one_hot_path([0] * 9 + [4], 5)
    assert stop_lengths(al, [5], 0, 1, 1)[0] == 10      # t* = Td - 1 = 9: 4 ceil(10 / 4) = 12, capped at Td = 10
    al = one_hot_path([4] * 10, 5)
    assert stop_lengths(al, [5], 0, 1, 11)[0] == 10     # min_steps = Td + 1 never fires
    assert stop_lengths(al, [5], 0, 11, 1)[0] == 10     # nor does a hold longer than Td
    assert stop_lengths(al, [5], 0, 10, 1)[0] == 10


def test_ties_take_the_lowest_index():
    al = np.zeros((1, 12, 6), dtype=np.float32)
    al[0, :, 2] = al[0, :, 5] = 0.5                      # a tie on every step: argmax 2, below target 5 -- never fires
    assert stop_lengths(al, [6], 0, 1, 1)[0] == 12
    al[0, :, 5] = 0.6                                    # 5 wins outright: fires on step 0
    assert stop_lengths(al, [6], 0, 1, 1)[0] == 4


def test_header_declares_the_entry_point():
    hdr = open(HDR).read()
    assert re.search(r'typedef struct TacoStopRule \{\s*int32_t end_offset;\s*int32_t hold;\s*int32_t min_steps;\s*int32_t reserved;\s*\}'
                     r' TacoStopRule;', hdr)
    decl = re.search(r'int taco_infer_stop\(([^)]*)\);', hdr)
    assert decl
    args = [a.strip() for a in decl.group(1).replace('\n', ' ').split(',')]
    assert args[5] == 'const TacoStopRule* rule' and args[9] == 'int32_t* lengths' and len(args) == 12
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120


def test_library_version(built_lib):
    assert built_lib.version() == 120
    assert built_lib.TacoStopRule(2, 3, 4).min_steps == 4 and built_lib.TacoStopRule().reserved == 0
