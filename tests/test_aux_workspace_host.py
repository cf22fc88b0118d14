"""CPU: every `*_workspace_bytes` function of the auxiliary entry points returns the byte count it has always returned.

The size functions and the entry points read one layout each (WsCarver, csrc/common.h), and callers size their buffers with these
numbers: a layout that is edited must not move a size.  CASES lists, per size function, the smallest accepted shape, the shapes one
below, at and one above every rounding or chunk boundary of its formula, the production shapes (B = 32; F = 360 and 720 frames;
L = 300 (F - 1) samples) and a few refused shapes.  tests/golden/aux_workspace_bytes.json holds what the library returned for each
of them at the commit in front of the one that introduced the layouts, negative return codes included; the test asserts equality.

  TACO_LIB=<that commit's libtaco_hip.so> python -m tests.test_aux_workspace_host --record      rewrites the golden file
"""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'aux_workspace_bytes.json')

_GL = [(1, 5), (2, 6), (1, 6), (3, 7), (32, 360), (32, 720), (1, 8192),
       (0, 5), (1, 4), (-1, 10)]
_DTW = [(1, 1, 1, 1), (2, 6, 5, 3),
        # diagonals + coefficients against 160 KiB of LDS: 24 Fa + 4 (Fa + Fb) (K | 1) <= 163840
        (2, 568, 568, 32), (2, 569, 568, 32), (2, 568, 569, 32), (2, 569, 569, 32),
        (1, 600, 600, 30), (1, 600, 600, 31), (1, 600, 600, 32),
        (1, 1024, 1024, 13), (1, 1024, 1024, 17), (1, 1024, 1024, 18), (1, 1024, 1024, 19), (1, 1024, 1024, 24), (1, 1024, 1024, 25),
        (1, 1024, 1024, 32), (1, 1, 1024, 32),
        (32, 360, 360, 13), (32, 720, 720, 13), (32, 720, 360, 13),
        (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 33), (1, 1025, 1, 1), (1, 1, 1025, 1)]

CASES = {
    'taco_griffinlim_workspace_bytes': _GL,
    'taco_griffinlim_rows_workspace_bytes': _GL,
    'taco_griffinlim_fast_workspace_bytes': _GL,
    # (B, L): L around multiples of 4, of 512 (the maxima's blocks and the trim hop) and of WF_CHUNK = 2048
    'taco_wave_finish_workspace_bytes': [
        (1, 1), (1, 3), (1, 4), (1, 5), (2, 7), (2, 8), (2, 9), (1, 511), (1, 512), (1, 513), (3, 1023), (3, 1024), (3, 1025),
        (1, 2047), (1, 2048), (1, 2049), (2, 4095), (2, 4096), (2, 4097), (32, 107700), (32, 215700),
        (0, 1), (1, 0), (-1, -1)],
    # (N, P, Lj): Lj around multiples of 4 and of a tile (Lj + 3 against WJ_T WJ_PER = 1024)
    'taco_wave_join_workspace_bytes': [
        (1, 1, 1), (1, 1, 3), (1, 1, 4), (1, 1, 5), (3, 2, 1020), (3, 2, 1021), (3, 2, 1022), (3, 2, 1023), (3, 2, 1024), (3, 2, 1025),
        (3, 2, 2045), (3, 2, 2046), (5, 1, 8), (64, 32, 215700), (96, 32, 431400),
        (0, 1, 1), (1, 0, 1), (1, 1, 0)],
    # (B, L, sr): L around multiples of 4, of WL_CHUNK = 2048 and of a hop of sr / 10 samples
    'taco_wave_loudness_workspace_bytes': [
        (1, 1, 8000), (1, 3, 16000), (1, 4, 16000), (1, 5, 16000), (2, 2047, 16000), (2, 2048, 16000), (2, 2049, 16000),
        (1, 799, 8000), (1, 800, 8000), (1, 801, 8000), (1, 1599, 8000), (1, 1600, 8000), (1, 1601, 8000),
        (1, 1599, 16000), (1, 1600, 16000), (1, 1601, 16000), (3, 3199, 16000), (3, 3200, 16000), (3, 3201, 16000),
        (1, 4799, 48000), (1, 4800, 48000), (1, 4801, 48000), (1, 9599, 48000), (1, 9600, 48000), (1, 2205, 22050), (1, 4410, 22050),
        (32, 107700, 16000), (32, 215700, 16000), (32, 215700, 24000),
        (0, 1, 16000), (1, 0, 16000), (1, 10, 7990), (1, 10, 16005), (1, 10, 48010)],
    # (B, L, W): L around LM_CHUNK = 2048; W = 0 and LM_WMAX = 512
    'taco_wave_limit_workspace_bytes': [
        (1, 1, 0), (1, 1, 512), (1, 2047, 0), (1, 2048, 0), (1, 2049, 0), (2, 2047, 24), (2, 2048, 24), (2, 2049, 24),
        (2, 4096, 512), (2, 4097, 512), (2, 4097, 1), (32, 107700, 24), (32, 215700, 24), (32, 215700, 0), (32, 215700, 512),
        (0, 1, 0), (1, 0, 0), (1, 1, -1), (1, 1, 513)],
    # (B, F): B F odd leaves 2 bytes behind the owners
    'taco_phase_estimate_workspace_bytes': [
        (1, 1), (1, 2), (1, 5), (3, 5), (2, 5), (1, 33), (3, 33), (2, 33), (1, 361), (32, 360), (32, 720),
        (0, 1), (1, 0)],
    # (B, C, F, lifter): F around the tile of 32 frames
    'taco_frames_cepstats_workspace_bytes': [
        (1, 9, 1, 2), (1, 17, 31, 2), (1, 17, 32, 2), (1, 17, 33, 2), (2, 17, 33, 8), (3, 1025, 63, 32), (3, 1025, 64, 32),
        (3, 1025, 65, 33), (1, 1025, 8192, 64), (32, 1025, 360, 32), (32, 1025, 720, 32),
        (0, 9, 1, 2), (1, 10, 1, 2), (1, 2049, 1, 2), (1, 9, 0, 2), (1, 9, 1, 1), (1, 9, 1, 5), (1, 1025, 8193, 32), (1, 1025, 10, 65)],
    # (B, L, F, K)
    'taco_f0_viterbi_workspace_bytes': [
        (1, 3, 1, 1), (1, 229, 33, 3), (2, 229, 33, 15), (32, 229, 360, 5), (32, 229, 720, 5), (1, 512, 8192, 15),
        (0, 3, 1, 1), (1, 2, 1, 1), (1, 513, 1, 1), (1, 3, 0, 1), (1, 3, 8193, 1), (1, 3, 1, 0), (1, 3, 1, 16)],
    # (n, n_items, nb): n_items records of 48 bytes around multiples of 64 bytes
    'taco_tensor_stats_workspace_bytes': [
        (1, 0, 3), (1, 1, 3), (1, 2, 3), (1, 3, 3), (1, 4, 3), (1, 5, 3), (3, 4, 33), (3, 5, 33), (3, 7, 33), (3, 8, 33), (3, 9, 33),
        (120, 1999, 129), (120, 2000, 129), (4096, 100000, 4065),
        (0, 1, 3), (4097, 1, 3), (1, -1, 3), (1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 1, 4067)],
    'taco_param_ema_workspace_bytes': [
        (1,), (1025,), (4096,), (7000000,), ((1 << 31) + 5,),
        (0,), (-1,)],
    # (B, L): the three arrays are rounded up to 256 bytes each: B around 64, B (1 + L / TRIM_HOP) around 64
    'taco_audio_features_workspace_bytes': [
        (1, 1), (1, 511), (1, 512), (1, 513), (63, 1), (64, 1), (65, 1), (2, 15871), (2, 15872), (2, 16383), (2, 16384),
        (32, 108000), (32, 215700),
        (0, 1), (1, 0)],
    'taco_frame_dtw_workspace_bytes': _DTW,
    'taco_frame_dtw_path_workspace_bytes': _DTW,
    # (B, Td, Tt): the single-wave form holds Tt <= 256 and a table of Td ceil(Tt / 4) words beside 4 Tt + 2 Td bytes in 128 KiB
    'taco_alignment_path_workspace_bytes': [
        (1, 1, 1), (2, 503, 256), (2, 504, 256), (2, 505, 256), (2, 504, 255), (2, 1, 257), (2, 9, 257), (1, 16384, 4), (1, 16384, 5),
        (1, 16384, 4096), (32, 144, 200), (32, 360, 256), (32, 720, 400),
        (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 16385, 1), (1, 1, 4097)],
}


def _call(lib, name, args):
    return int(getattr(lib._lib, name)(*args))


def test_cases_cover_accepted_and_refused_shapes():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(CASES)
    for name, rows in golden.items():
        assert [tuple(r[:-1]) for r in rows] == CASES[name], name
        values = [r[-1] for r in rows]
        assert any(v >= 0 for v in values) and any(v < 0 for v in values), name


@pytest.mark.parametrize('name', sorted(CASES))
def test_size_is_the_recorded_one(built_lib, name):
    golden = json.load(open(GOLDEN))[name]
    got = [list(args) + [_call(built_lib, name, args)] for args in CASES[name]]
    assert got == golden


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], __doc__
    from tacotron_amd import lib
    out = {name: [list(args) + [_call(lib, name, args)] for args in rows] for name, rows in CASES.items()}
    with open(GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(' %s: [\n%s]' % (json.dumps(k), ',\n'.join('  ' + json.dumps(r) for r in v))
                                   for k, v in sorted(out.items())) + '\n}\n')
    print('wrote %s from %s' % (GOLDEN, lib.LIB_PATH))
