"""The drivers of the alignment path on the GPU: tacotron_amd.test.test(timings=True) with a stop rule, with a stop rule and a rate,
with a trim, and with `long` on a prompt of two pieces -- the duration files and the word tables against alignment.word_times of
the saved alignments through the restatement (tests/align_path_ref.py), every other file byte for byte what the run without
`timings` writes -- and tacotron_amd.evaluate.evaluate(durations=True) on the synthetic pool.  An untrained model at the shapes of the
other driver tests: the paths follow no text, the arithmetic is what is checked."""
import os

import numpy as np
import pytest

from tests import align_path_ref as pr

pytestmark = pytest.mark.gpu

RULE = dict(end_offset=200, hold=1, min_steps=5)   # target 0: every row stops after step 4 -> len_b = 8
PROMPTS = ['hello world.\n', 'A somewhat longer prompt, with punctuation!\n']   # ('A' is outside the vocabulary: dropped)
TWO = ('the first sentence of this prompt is long enough to fill a good part of one piece on its own, and it ends here. '
       'the second one follows it, and with it the line has well over one hundred and forty characters.\n')
IVOCAB = {i + 1: ch for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz '.,?!-")}
IVOCAB[0] = '<pad>'


def _cfg(tmp_path):
    from tacotron_amd.config import Config
    c = Config()
    c.data_path = str(tmp_path / 'no_data') + '/'
    c.max_decode_iter = 16
    return c


def _files(d):
    return {name: open(os.path.join(d, name), 'rb').read() for name in sorted(os.listdir(d))}


def _pair(tmp_path, prompts, **options):
    """the same run without and with timings -> (files without, files with, stdout lines the timings added)"""
    import contextlib
    import io
    from tacotron_amd import test as drv
    outs = []
    for sub, extra in (('plain', {}), ('timed', dict(timings=True))):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            assert drv.test(_cfg(tmp_path), prompts, out_dir=str(tmp_path / sub), n_iter=2, **options, **extra) == len(prompts)
        outs.append(buf.getvalue().splitlines())
    plain, timed = _files(tmp_path / 'plain'), _files(tmp_path / 'timed')
    added = [line for line in outs[1] if ' path: ' in line]
    assert [line for line in outs[1] if line not in added] == [line.replace('plain', 'timed') for line in outs[0]]
    for name, data in plain.items():
        assert timed[name] == data, name + ' changed with timings'
    return plain, timed, added


def _expect(lib, d, stem, line, jump=None, **mapping):
    """(dur, word rows) of the piece saved as `stem`, from its saved alignment through the restatement"""
    from tacotron_amd.alignment import word_times
    al = np.load(os.path.join(d, stem + '_align.npy'))
    L = min(len(line), 140)
    path, dur, counts, mass = pr.best_path(al, L, None, lib.PATH_JUMP if jump is None else jump)
    assert dur[:L].sum() == al.shape[0] and (dur[L:] == 0).all()
    return dur[:L], word_times(line, IVOCAB, dur[:L], 2, **mapping), counts


def _check_prompt(lib, d, i, line, added, **mapping):
    from tacotron_amd.alignment import path_line, words_tsv
    stem = 'prompt_%03d' % i
    dur, words, counts = _expect(lib, d, stem, line, **mapping)
    got = np.load(os.path.join(d, stem + '_dur.npy'))
    assert got.dtype == np.int32 and got.shape == (min(len(line), 140),) and np.array_equal(got, dur)
    assert open(os.path.join(d, stem + '_words.tsv')).read() == words_tsv(words)
    spoken = [w for w in line.split() if any(ch in IVOCAB.values() for ch in w)]
    assert len(words) == len(spoken) and all(0.0 <= a <= b for a, b, _ in words)
    mine = [x for x in added if x.startswith('prompt %d path: ' % i) or x.startswith('WARNING prompt %d path: ' % i)]
    assert len(mine) == 1 and 'over %d steps, end %d of %d, %d skipped' % (counts[0], counts[1], min(len(line), 140) - 1, counts[2]) in mine[0]
    return words


def test_timings_with_a_stop_rule(built_lib, tmp_path):
    lib = built_lib
    assert _cfg(tmp_path).r == 2
    plain, timed, added = _pair(tmp_path, PROMPTS, stop=lib.TacoStopRule(**RULE))
    assert sorted(set(timed) - set(plain)) == sorted('prompt_%03d_%s' % (i, k) for i in range(2) for k in ('dur.npy', 'words.tsv'))
    assert len(added) == 2 and not any(x.startswith('WARNING') for x in added)       # (end_offset 200: no path ends too early)
    for i, line in enumerate(PROMPTS):
        assert int(np.load(tmp_path / 'timed' / ('prompt_%03d_len.npy' % i))) == 8
        words = _check_prompt(lib, tmp_path / 'timed', i, line, added, total=300 * (8 * 2 - 1))
        assert max(b for _, b, _ in words) <= 300 * 15 / 16000.0
    assert [w for _, _, w in words] == ['somewhat', 'longer', 'prompt,', 'with', 'punctuation!']


def test_timings_with_a_stop_rule_and_a_rate(built_lib, tmp_path):
    lib = built_lib
    plain, timed, added = _pair(tmp_path, PROMPTS, stop=lib.TacoStopRule(**RULE), rate=[0.5, 2.0])
    assert len(timed) == len(plain) + 4
    for i, (line, q) in enumerate(zip(PROMPTS, (32768, 131072))):
        step_q, Fob = np.load(tmp_path / 'timed' / ('prompt_%03d_rate.npy' % i)).tolist()
        assert step_q == q and Fob == lib.stretch_frames(16, q)
        _check_prompt(lib, tmp_path / 'timed', i, line, added, step_q=q, total=300 * (Fob - 1))


def test_timings_with_a_trim(built_lib, tmp_path):
    lib = built_lib
    plain, timed, added = _pair(tmp_path, PROMPTS, trim_db=25.0)
    assert len(timed) == len(plain) + 4
    for i, line in enumerate(PROMPTS):
        trim = np.load(tmp_path / 'timed' / ('prompt_%03d_trim.npy' % i))
        assert np.load(tmp_path / 'timed' / ('prompt_%03d_align.npy' % i)).shape == (16, 140)
        words = _check_prompt(lib, tmp_path / 'timed', i, line, added, trim=trim)
        assert max(b for _, b, _ in words) <= (trim[1] - trim[0]) / 16000.0


def test_timings_with_long_on_a_prompt_of_two_pieces(built_lib, tmp_path):
    from tacotron_amd import data
    from tacotron_amd.alignment import words_tsv
    lib = built_lib
    pieces = data.split_prompt(TWO)
    assert len(pieces) == 2
    plain, timed, added = _pair(tmp_path, [PROMPTS[0], TWO], stop=lib.TacoStopRule(**RULE), long=True, path_jump=2)
    d = tmp_path / 'timed'
    assert sorted(set(timed) - set(plain)) == ['prompt_000_dur.npy', 'prompt_000_words.tsv', 'prompt_001_k00_dur.npy',
                                               'prompt_001_k01_dur.npy', 'prompt_001_words.tsv']
    # the prompt of one piece: the files it writes without `long`, its trim applied
    dur, words, _ = _expect(lib, d, 'prompt_000', PROMPTS[0], jump=2, trim=np.load(d / 'prompt_000_trim.npy'))
    assert np.array_equal(np.load(d / 'prompt_000_dur.npy'), dur) and open(d / 'prompt_000_words.tsv').read() == words_tsv(words)
    # the prompt of two: a duration file per piece, one table with the pieces' offsets in the joined file
    table = np.load(d / 'prompt_001_pieces.npy')
    assert table.shape == (2, 4) and table[0, 0] == 0 and table[1, 0] > 0
    rows = []
    for k, (line, _) in enumerate(pieces):
        stem = 'prompt_001_k%02d' % k
        dur, words, _ = _expect(lib, d, stem, line, jump=2, trim=np.load(d / (stem + '_trim.npy')), offset=int(table[k, 0]))
        assert np.array_equal(np.load(d / (stem + '_dur.npy')), dur)
        assert all(a >= table[k, 0] / 16000.0 and b <= (table[k, 0] + table[k, 1]) / 16000.0 for a, b, _ in words)
        rows += words
    assert open(d / 'prompt_001_words.tsv').read() == words_tsv(rows) and len(rows) == len(TWO.split())
    assert sorted(x.split(' path: ')[0] for x in added) == ['prompt 0', 'prompt 1 piece 0', 'prompt 1 piece 1']


def test_evaluate_durations(built_lib, tmp_path, capsys):
    """evaluate(durations=True) on the synthetic pool: DUR_COLUMNS behind the columns of the run without it, which stay what they were,
    and equal to the restatement of both alignments over free.lengths and over the recording's own steps"""
    from tacotron_amd import evaluate as ev
    from tacotron_amd.config import Config
    lib = built_lib

    def cfg():
        c = Config()
        c.data_path = str(tmp_path / 'no_data') + '/'
        c.batch_size, c.max_decode_iter = 3, 12
        return c

    plain, loss = ev.evaluate(cfg(), 5, out_dir=str(tmp_path / 'plain'))
    plain_out = capsys.readouterr().out.splitlines()
    trace = []
    rows, loss2 = ev.evaluate(cfg(), 5, out_dir=str(tmp_path / 'dur'), durations=True, trace=trace)
    out = capsys.readouterr().out.splitlines()
    assert rows.shape == (5, len(ev.COLUMNS) + len(ev.DUR_COLUMNS)) and np.array_equal(rows[:, :6], plain, equal_nan=True) and loss2 == loss
    added = [line for line in out if 'duration error' in line]
    assert len(added) == 3 and added[-1].startswith('held out: duration error') and [line for line in out if line not in added] == plain_out
    assert np.array_equal(np.load(tmp_path / 'dur' / 'eval_0.npy'), rows, equal_nan=True)
    assert np.array_equal(np.load(tmp_path / 'plain' / 'eval_0.npy'), plain, equal_nan=True)
    r = cfg().r
    want = []
    for (index, valid), t in zip(ev.holdout_batches(256, 5, 3), trace):
        Td = t['rec_alignments'].shape[1]
        assert t['rec_steps'].tolist() == [min(Td, 4 * -(-int(nb) // (4 * r))) for nb in t['nb']]
        free = pr.best_paths(t['alignments'], t['text_length'], t['lengths'], lib.PATH_JUMP)
        rec = pr.best_paths(t['rec_alignments'], t['text_length'], t['rec_steps'], lib.PATH_JUMP)
        want.append(ev.duration_columns(free[1], rec[1], t['text_length'], free[2], free[3], rec[2], rec[3], 1000.0 * r * 300 / 16000)[:valid])
    assert np.array_equal(rows[:, 6:], np.concatenate(want), equal_nan=True)
    assert np.isfinite(rows[:, 6:8]).all() and (rows[:, 6] >= np.abs(rows[:, 7])).all()
