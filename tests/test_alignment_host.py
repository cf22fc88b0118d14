"""CPU checks of the alignment monitor (taco_alignment_scores): the C ABI declaration and its version, the export and its ctypes
signature, every TACO_EINVAL case of the library and every refusal of the Python binding, alignment.flags on hand-made rows,
alignment.attention_png against the restatement (tests/align_ref.py) and against matplotlib where it is installed, the restatement of
the scores on numbers worked by hand, and the two drivers' options."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import align_ref as ar

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'taco_hip.h')


def _args(decl):
    return [' '.join(a.split()) for a in decl.replace('\n', ' ').split(',')]


def test_header_declares_the_entry_point():
    hdr = open(HDR).read()
    fn = re.search(r'\bint taco_alignment_scores\(([^)]*)\);', hdr)
    assert fn
    assert _args(fn.group(1)) == ['const float* alignments', 'const int32_t* text_length', 'const int32_t* steps', 'int max_jump',
                                  'int32_t* counts', 'float* means', 'int B', 'int Td', 'int Tt', 'void* stream']
    at = [hdr.index(d) for d in ('int taco_infer_stop(', 'int taco_alignment_scores(', 'int taco_clip_adam_step(')]
    assert at == sorted(at)
    assert int(re.search(r'#define\s+TACO_VERSION\s+(\d+)', hdr).group(1)) == 120
    limits = {k: int(re.search(r'#define\s+%s\s+(\d+)' % k, hdr).group(1)) for k in ('TACO_ALIGNMENT_MAX_TD', 'TACO_ALIGNMENT_MAX_TT')}
    assert limits['TACO_ALIGNMENT_MAX_TD'] >= 4096 and limits['TACO_ALIGNMENT_MAX_TT'] >= 1024
    comment = ' '.join(hdr[hdr.index('/* Alignment scores'):fn.start()].split())
    for word in ('pad_steps', 'back', 'skip', 'covered', 'focus', 'pad_mass', 'NaN', 'detect it by the symbol', 'graph-capturable'):
        assert word in comment, word


def test_library_exports_it_at_version_120(built_lib):
    assert built_lib.version() == 120
    assert 'taco_alignment_scores' in built_lib.EXPORTS
    assert hasattr(C.CDLL(built_lib.LIB_PATH), 'taco_alignment_scores')
    P, I = C.c_void_p, C.c_int
    assert built_lib.EXPORTS['taco_alignment_scores'] == (C.c_int, [P, P, P, I, P, P, I, I, I, P])
    assert built_lib.ALIGN_COUNTS == ('n', 'end', 'pad_steps', 'back', 'skip', 'covered')
    assert built_lib.ALIGN_MEANS == ('focus', 'pad_mass')
    hdr = open(HDR).read()
    assert built_lib.ALIGN_MAX_TD == int(re.search(r'TACO_ALIGNMENT_MAX_TD\s+(\d+)', hdr).group(1))
    assert built_lib.ALIGN_MAX_TT == int(re.search(r'TACO_ALIGNMENT_MAX_TT\s+(\d+)', hdr).group(1))


def test_library_refuses_bad_arguments(built_lib):
    """every TACO_EINVAL case, at the library itself: rc -1 and a message that names the argument.  The refusals come before the
    launch, so host memory stands in for the device buffers and nothing of it changes."""
    B, Td, Tt = 2, 3, 5
    al = np.full(B * Td * Tt, 0.25, dtype=np.float32)
    tl = np.full(B, 4, dtype=np.int32)
    counts = np.full(B * 6, -7, dtype=np.int32)
    means = np.full(B * 2, -7.0, dtype=np.float32)
    p = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    good = dict(al=p(al), tl=p(tl), steps=None, max_jump=2, counts=p(counts), means=p(means), B=B, Td=Td, Tt=Tt)
    fn = built_lib._lib.taco_alignment_scores
    cases = [(dict(al=None), 'alignments'), (dict(tl=None), 'text_length'), (dict(counts=None), 'counts'), (dict(means=None), 'means'),
             (dict(B=0), 'B='), (dict(B=-1), 'B='), (dict(Td=0), 'Td='), (dict(Td=-4), 'Td='), (dict(Tt=0), 'Tt='), (dict(Tt=-1), 'Tt='),
             (dict(max_jump=-1), 'max_jump'), (dict(Td=built_lib.ALIGN_MAX_TD + 1), 'Td='), (dict(Tt=built_lib.ALIGN_MAX_TT + 1), 'Tt=')]
    for kw, word in cases:
        a = dict(good, **kw)
        rc = fn(a['al'], a['tl'], a['steps'], a['max_jump'], a['counts'], a['means'], a['B'], a['Td'], a['Tt'], None)
        assert rc == -1, kw
        msg = built_lib.last_error()
        assert msg.startswith('alignment_scores:') and word in msg, (kw, msg)
    assert (counts == -7).all() and (means == -7.0).all() and (al == 0.25).all() and (tl == 4).all()


def test_wrapper_refuses_bad_arguments_before_any_device_call(built_lib):
    """every refusal is raised on the host before the entry point is called (CPU tensors never reach it)"""
    B, Td, Tt = 3, 4, 6
    al = torch.zeros(B, Td, Tt)
    tl = torch.ones(B, dtype=torch.int32)
    good = dict(alignments=al, text_length=tl)
    called = []
    real = built_lib._lib.taco_alignment_scores
    bad = [
        dict(alignments=al.double()), dict(alignments=al.half()), dict(alignments=torch.zeros(Td, Tt)), dict(alignments=torch.zeros(B, 0, Tt)),
        dict(alignments=torch.zeros(B, Tt, Td).transpose(1, 2)),                      # not contiguous
        dict(alignments=np.zeros((B, Td, Tt), dtype=np.float32)),                     # not a tensor
        dict(alignments=torch.zeros(1, 1, 1).expand(1, built_lib.ALIGN_MAX_TD + 1, 1)),
        dict(text_length=None), dict(text_length=tl.long()), dict(text_length=torch.ones(B + 1, dtype=torch.int32)),
        dict(text_length=[1, 1, 1]),
        dict(steps=torch.ones(B)), dict(steps=torch.ones(B - 1, dtype=torch.int32)), dict(steps=[4, 4, 4]),
        dict(max_jump=-1), dict(max_jump=1.5), dict(max_jump=True), dict(max_jump=1 << 31),
        dict(counts=torch.zeros(B, 6)), dict(counts=torch.zeros(B, 5, dtype=torch.int32)), dict(counts=torch.zeros(B + 1, 6, dtype=torch.int32)),
        dict(means=torch.zeros(B, 2, dtype=torch.float64)), dict(means=torch.zeros(B, 3)), dict(means=torch.zeros(2, B).t()),
        dict(),                                                                       # everything right, but on the CPU
    ]
    try:
        built_lib._lib.taco_alignment_scores = lambda *a: called.append(a) or 0
        for kw in bad:
            with pytest.raises(ValueError):
                built_lib.alignment_scores(**dict(good, **kw))
    finally:
        built_lib._lib.taco_alignment_scores = real
    assert not called
    sig = inspect.signature(built_lib.alignment_scores).parameters
    assert [(k, sig[k].default) for k in list(sig)[2:]] == [('steps', None), ('max_jump', built_lib.MAX_JUMP), ('counts', None),
                                                            ('means', None)]
    assert built_lib.MAX_JUMP == ar.MAX_JUMP >= 0


# ---- the restatement on numbers worked by hand -------------------------------------------------------------------------------------
def test_restatement_on_hand_numbers():
    nan = np.nan
    al = np.array([[[0.1, 0.7, 0.7, 0.0],      # tie: the lower index
                    [0.9, 0.0, 0.1, 0.0],      # back by one
                    [0.0, 0.0, 0.2, 0.8],      # +3: a skip for max_jump 2, on padding for L = 3
                    [nan, nan, nan, nan],      # every element NaN: a_t = 0
                    [nan, 0.3, 0.1, nan]]],    # NaN elements never win
                  dtype=np.float32)
    c, m = ar.scores(al, [3], None, 2)
    assert c.tolist() == [[5, 3, 1, 2, 1, 2]]   # back: 1 -> 0 and 3 -> 0; skip: 0 -> 3; covered {1, 0}
    assert np.isnan(m).all()
    c, m = ar.scores(al, [3], [3], 2)
    assert c.tolist() == [[3, 3, 1, 1, 1, 2]]
    assert m[0, 0] == pytest.approx((float(np.float32(0.7)) + float(np.float32(0.9)) + float(np.float32(0.8))) / 3, abs=1e-12)
    assert m[0, 1] == pytest.approx(float(np.float32(0.8)) / 3, abs=1e-12)
    c, m = ar.scores(al, [0], [-2], 2)          # L clamps to 1, n to 0
    assert c.tolist() == [[0, 0, 0, 0, 0, 0]] and m.tolist() == [[0.0, 0.0]]
    c, _ = ar.scores(al, [9], [99], 3)          # L clamps to Tt, n to Td; +3 is no skip for max_jump 3
    assert c.tolist() == [[5, 3, 0, 2, 0, 3]]
    assert ar.means_bound(180, 200) == 380 * 2.0 ** -23


# ---- flags -----------------------------------------------------------------------------------------------------------------------
def test_flags_on_hand_made_rows(built_lib):
    from tacotron_amd import alignment as A
    L = 20
    fine = ([60, 19, 0, 0, 0, 20], [0.9, 0.0])
    assert A.flags(*fine, L) == []
    assert A.flags([60, 18, 0, 0, 0, 16], [0.9, 0.0], L) == []                      # the stop rule's target (L - 2), 0.8 L covered
    assert A.flags([60, 17, 0, 0, 0, 20], [0.9, 0.0], L) == ['unfinished']          # end below the target
    assert A.flags([60, 17, 0, 0, 0, 20], [0.9, 0.0], L, end_offset=2) == []
    assert A.flags([60, 19, 0, 0, 0, 15], [0.9, 0.0], L) == ['unfinished']          # covered < 0.8 L
    assert A.flags([60, 19, 0, 0, 3, 20], [0.9, 0.0], L) == ['skips']
    assert A.flags([60, 19, 0, 0, 2, 20], [0.9, 0.0], L) == []
    assert A.flags([60, 19, 0, 3, 0, 20], [0.9, 0.0], L) == ['goes back']
    assert A.flags([60, 19, 7, 0, 0, 20], [0.9, 0.0], L) == ['on padding']          # more than a tenth of the steps
    assert A.flags([60, 19, 6, 0, 0, 20], [0.9, 0.0], L) == []
    assert A.flags([60, 19, 0, 0, 0, 20], [0.9, 0.2], L) == ['on padding']          # the mass
    assert A.flags([60, 19, 0, 0, 0, 20], [0.2, 0.0], L) == ['diffuse']
    assert A.flags([60, 19, 0, 0, 0, 20], [float('nan'), float('nan')], L) == ['on padding', 'diffuse']
    assert A.flags([0, 0, 0, 0, 0, 0], [0.0, 0.0], L) == ['unfinished']             # a row of no steps
    assert A.flags([60, 3, 30, 9, 9, 2], [0.05, 0.6], L) == list(A.FLAGS)           # everything at once, in the order of FLAGS
    assert A.flags([60, 19, 0, 5, 5, 20], [0.9, 0.0], L, max_skip=5, max_back=5) == []
    assert A.flags(np.array(fine[0], dtype=np.int32), np.array(fine[1], dtype=np.float32), np.int32(L)) == []
    defaults = {k: v.default for k, v in inspect.signature(A.flags).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(end_offset=1, min_covered=0.8, max_skip=2, max_back=2, max_pad_steps=0.1, max_pad_mass=0.1, min_focus=0.3)
    assert 'none is tuned on a trained model' in ' '.join(A.flags.__doc__.split())
    row = A.scores_row(fine[0], np.array(fine[1], dtype=np.float32))
    assert row.dtype == np.float64 and row.tolist() == [60, 19, 0, 0, 0, 20, float(np.float32(0.9)), 0.0]
    with pytest.raises(ValueError):
        A.scores_row(fine[0][:5], fine[1])


# ---- the picture -------------------------------------------------------------------------------------------------------------------
def test_attention_png_pixels_equal_the_restatement(built_lib, tmp_path):
    from tacotron_amd import alignment as A
    assert np.array_equal(A.hot_table(), ar.hot_table()) and A.hot_table().shape == (256, 3) and A.hot_table().dtype == np.uint8
    assert A.hot_table()[0].tolist() == [10, 0, 0] and A.hot_table()[255].tolist() == [255, 255, 255]
    rng = np.random.default_rng(5)
    a = (rng.random((9, 13)) ** 4).astype(np.float32)
    a[0, 0], a[8, 12] = 0.0, 1.0
    path = str(tmp_path / 'a.png')
    assert A.attention_png(path, a) == (36, 52)
    got = ar.read_png(path)
    assert got.shape == (36, 52, 3) and np.array_equal(got, ar.pixels(a))
    assert got[0, 0].tolist() == [10, 0, 0] and got[35, 51].tolist() == [255, 255, 255]
    # n rows from the top, another zoom: the range is that of the drawn cells only
    assert A.attention_png(path, a, n=5, zoom=3) == (15, 39)
    got = ar.read_png(path)
    assert np.array_equal(got, ar.pixels(a, 5, 3)) and not np.array_equal(got, ar.pixels(a, 9, 3)[:15])
    assert A.attention_png(path, a, n=1, zoom=1) == (1, 13) and np.array_equal(ar.read_png(path), ar.pixels(a, 1, 1))
    # a constant picture and NaN cells take index 0
    A.attention_png(path, np.full((3, 4), 0.25, dtype=np.float32), zoom=2)
    assert (ar.read_png(path) == np.array([10, 0, 0], dtype=np.uint8)).all()
    b = a.copy()
    b[2, 3] = b[8, 12] = np.nan
    A.attention_png(path, b, zoom=2)
    got = ar.read_png(path)
    assert np.array_equal(got, ar.pixels(b, None, 2)) and got[4, 6].tolist() == [10, 0, 0] and got[17, 25].tolist() == [10, 0, 0]
    A.attention_png(path, np.full((2, 2), np.nan, dtype=np.float32), zoom=1)
    assert (ar.read_png(path) == np.array([10, 0, 0], dtype=np.uint8)).all()
    for kw in (dict(n=0), dict(n=10), dict(zoom=0)):
        with pytest.raises(ValueError):
            A.attention_png(path, a, **kw)
    with pytest.raises(ValueError):
        A.attention_png(path, a[0])


def test_attention_png_is_matplotlibs_hot(built_lib):
    matplotlib = pytest.importorskip('matplotlib')
    from matplotlib.colors import Normalize
    from tacotron_amd import alignment as A
    hot = matplotlib.colormaps['hot']
    assert np.array_equal(A.hot_table(), hot(np.arange(256), bytes=True)[:, :3])
    rng = np.random.default_rng(9)
    for shape in ((180, 200), (7, 5)):
        a = (rng.random(shape) ** 3).astype(np.float32)
        assert np.array_equal(A.attention_pixels(a, zoom=1), hot(Normalize()(a), bytes=True)[..., :3])


# ---- the drivers' options ----------------------------------------------------------------------------------------------------------
def test_driver_options(built_lib, capsys, tmp_path):
    from tacotron_amd import test as drv, train as trn
    assert drv.parse_args([]).align_scores is False
    assert drv.parse_args(['--align-scores']).align_scores is True
    a = drv.parse_args(['--stop', '--long', '--vocode-lengths', '--deemphasis', '--align-scores'])
    assert a.align_scores and a.stop and a.vocode_lengths and a.long is not None and a.deemphasis == 0.97
    assert inspect.signature(drv.test).parameters['align_scores'].default is False
    d = inspect.signature(drv.write_prompt).parameters
    assert d['ascore'].default is None and d['zoom'].default == 4
    assert trn.parse_args([]).align_log is False and trn.parse_args(['--align-log', '--steps', '5']).align_log is True
    assert inspect.signature(trn.train).parameters['align_log'].default is False
    assert inspect.signature(trn.save_sample).parameters['align'].default is False
    capsys.readouterr()
    for mod in (drv, trn):
        with pytest.raises(SystemExit):
            mod.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--align-scores' in text and '--align-log' in text and text.count('untuned') >= 2
    # write_prompt: the defaults write today's files; ascore adds the two new ones
    spec, al = np.zeros((8, 1025), dtype=np.float32), np.random.default_rng(1).random((4, 6)).astype(np.float32)
    drv.write_prompt(str(tmp_path), 0, 2, spec, al)
    assert sorted(os.listdir(tmp_path)) == ['prompt_000_align.npy', 'prompt_000_spec.npy']
    drv.write_prompt(str(tmp_path), 1, 2, spec, al, len_b=3, piece=2, ascore=np.arange(8))
    new = sorted(set(os.listdir(tmp_path)) - {'prompt_000_align.npy', 'prompt_000_spec.npy'})
    assert new == ['prompt_001_k02_align.npy', 'prompt_001_k02_align.png', 'prompt_001_k02_ascore.npy', 'prompt_001_k02_len.npy',
                   'prompt_001_k02_spec.npy']
    got = np.load(tmp_path / 'prompt_001_k02_ascore.npy')
    assert got.dtype == np.float64 and got.tolist() == list(range(8))
    assert np.array_equal(ar.read_png(str(tmp_path / 'prompt_001_k02_align.png')), ar.pixels(al, 3, 4))
    # the training log line
    counts = np.array([[10, 4, 0, 1, 0, 5], [10, 9, 5, 3, 4, 2]])
    means = np.array([[0.9, 0.0], [0.1, 0.5]], dtype=np.float32)
    line = trn.align_line(counts, means, np.array([5, 40]), Tt=10)   # (40 clamps to Tt = 10)
    assert line == 'align focus 0.500 covered 0.600 back 2.00 skip 2.00 pad_mass 0.2500 flagged 1/2'
