"""CPU: the row plan of the listed-row GEMMs (rnn_util.valid_rows / row_plans) against a brute-force loop.  A plan lists
the valid frames {t * B + b : t < len_b} of a time-major [T, B] layout, ascending; a batch cut into two pipelines gets one
plan per part, each in that part's own layout."""
import numpy as np
import pytest

from tensorflow_end2end_speech_recognition_amd.models.encoders.core import rnn_util


def _brute(lens, T, B):
    out = []
    for t in range(T):
        for b in range(B):
            if b < len(lens) and t < lens[b]:
                out.append(t * B + b)
    return out


T = 37
CASES = {
    'all_equal': [T] * 16,
    'one_full_rest_ragged': [T, 5, 12, 36, 1, 20, 9, 30, 2, 17, 33, 8, 25, 11, 3, 19],
    'a_length_of_one': [1] + [T] * 15,
    'only_ones': [1] * 16,
    'zero_length_padding_rows': [T, 4, 0, 0, 9, 0, 36, 1, 0, 0, 0, 0, 0, 0, 0, 0],
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_valid_rows_matches_the_brute_force_loop(name):
    lens = CASES[name]
    rows = rnn_util.valid_rows(lens, T)
    assert rows.dtype == np.int32 and rows.ndim == 1
    assert rows.tolist() == _brute(lens, T, len(lens))
    assert rows.size == sum(lens)
    assert np.all(np.diff(rows) > 0)


def test_batch_padding_rows_contribute_nothing():
    lens = [T, 7, 1, 20, 13]                       # five utterances in a 16-row tile
    rows = rnn_util.valid_rows(lens, T, B=16)
    assert rows.tolist() == _brute(lens, T, 16)
    assert rows.size == sum(lens)
    with pytest.raises(ValueError):
        rnn_util.valid_rows(lens, T, B=4)


def test_lengths_are_clamped_to_the_frame_count():
    assert rnn_util.valid_rows([T + 5, -3, 2], T).tolist() == _brute([T, 0, 2], T, 3)


def test_two_pipelines_get_one_plan_each_in_their_own_layout(monkeypatch):
    monkeypatch.setattr(rnn_util, 'VALID_ROWS', True)
    rng = np.random.RandomState(3)
    lens = rng.randint(0, T + 1, size=32)
    lens[0], lens[17], lens[5], lens[30] = T, T, 1, 0
    one = rnn_util.row_plans(lens, 32, T, 32)
    assert len(one) == 1 and one[0].tolist() == _brute(lens, T, 32)
    a, b = rnn_util.row_plans(lens, 32, T, 32, split=16)
    assert a.tolist() == _brute(lens[:16], T, 16) and a.size == int(lens[:16].sum())
    assert b.tolist() == _brute(lens[16:], T, 16) and b.size == int(lens[16:].sum())
    for p in (a, b):
        assert p.dtype == np.int32 and np.all(np.diff(p) > 0)
    # B = 20 padded to 32: the second part is four utterances and twelve zero-length rows
    a, b = rnn_util.row_plans(lens[:20], 20, T, 32, split=16)
    assert a.tolist() == _brute(lens[:16], T, 16)
    assert b.tolist() == _brute(lens[16:20], T, 16) and b.size == int(lens[16:20].sum())


def test_no_plan_without_matching_host_lengths_or_with_the_switch_off(monkeypatch):
    monkeypatch.setattr(rnn_util, 'VALID_ROWS', True)
    assert rnn_util.row_plans(None, 16, T, 16) is None
    assert rnn_util.row_plans([T] * 15, 16, T, 16) is None          # lengths of another batch
    assert rnn_util.row_plans([T] * 16, 16, T, 16) is not None
    monkeypatch.setattr(rnn_util, 'VALID_ROWS', False)
    assert rnn_util.row_plans([T] * 16, 16, T, 16) is None
