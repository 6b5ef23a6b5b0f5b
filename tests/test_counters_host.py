"""The launch-counter table (_counters.py) on the host: held to include/asr_hip.h (word counts of every family), to the
ctypes binding (_lib.SIGNATURES) and to the public functions of ops built from it -- a key added on one side only would
mislabel every counter behind it."""
import ctypes as C
import inspect
import os
import re

import pytest

import _cpu_ops_weight_noise as wn_ops
from tensorflow_end2end_speech_recognition_amd import _counters, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the sized families: the enumerator that closes the enum their words are indexed by
SIZED_N = {'lstm_kernel_counts': 'ASR_LSTM_KERNEL_N', 'att_path_counts': 'ASR_ATT_PATH_N',
           'conv_path_counts': 'ASR_CONVP_N', 'gemm_path_counts': 'ASR_GEMMP_N'}


def _header():
    src = open(os.path.join(ROOT, 'include', 'asr_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def _enum_length(src, last):
    """Enumerators in front of `last` in the enum whose last enumerator it is."""
    found = []
    for body in re.findall(r'\benum\s*\w*\s*\{([^}]*)\}', src):
        names = [e.split('=')[0].strip() for e in body.split(',') if e.strip()]
        if names and names[-1] == last:
            found.append(len(names) - 1)
    assert len(found) == 1, (last, found)
    return found[0]


def test_table_matches_header():
    src = _header()
    assert sorted(f for f, fam in _counters.FAMILIES.items() if fam.sized) == sorted(SIZED_N)
    for name, fam in _counters.FAMILIES.items():
        assert fam.getter == 'asr_' + name and fam.reset == 'asr_reset_' + name
        assert re.search(r'\bint %s\(asr_handle\* h\);' % fam.reset, src), fam.reset
        if fam.sized:
            assert re.search(r'\bint %s\(asr_handle\* h, unsigned long long\* out, int n\);' % fam.getter, src), fam.getter
            words = _enum_length(src, SIZED_N[name])
        else:
            m = re.search(r'\bint %s\(asr_handle\* h, unsigned long long\* out(\d+)\);' % fam.getter, src)
            assert m, fam.getter
            words = int(m.group(1))
        assert len(fam.keys) == words, (name, len(fam.keys), words)
    # and the header declares no counter family that the table lacks
    declared = set(re.findall(r'\bint (asr_(?:reset_)?\w+_counts)\(', src))
    assert declared == {n for fam in _counters.FAMILIES.values() for n in (fam.getter, fam.reset)}


def test_table_matches_signatures():
    u64p = C.POINTER(C.c_ulonglong)
    for fam in _counters.FAMILIES.values():
        assert _lib.SIGNATURES[fam.getter] == (C.c_int, [C.c_void_p, u64p] + ([C.c_int] if fam.sized else [])), fam.getter
        assert _lib.SIGNATURES[fam.reset] == (C.c_int, [C.c_void_p]), fam.reset
    bound = {n for n in _lib.SIGNATURES if n.endswith('_counts')}
    assert bound == {n for fam in _counters.FAMILIES.values() for n in (fam.getter, fam.reset)}


def test_views_tile_their_families():
    by_family = {}
    for name, v in _counters.VIEWS.items():
        assert v.name == name and v.family in _counters.FAMILIES
        assert len(set(v.keys)) == len(v.keys) > 0, name
        by_family.setdefault(v.family, []).append(v)
    assert set(by_family) == set(_counters.FAMILIES)
    for family, views in by_family.items():
        keys, at = _counters.FAMILIES[family].keys, 0
        for v in sorted(views, key=lambda v: v.offset):
            assert v.offset == at, (v.name, v.offset, at)                   # no gap, no overlap
            assert v.keys == keys[at:at + len(v.keys)], v.name
            at += len(v.keys)
        assert at == len(keys), family
        assert sum(v.reset is not None for v in views) == 1, family        # one reset per family
    resets = [v.reset for v in _counters.VIEWS.values() if v.reset]
    assert len(set(resets)) == len(resets)


def test_public_names_are_plain_assignments_in_ops():
    text = inspect.getsource(ops)
    for v in _counters.VIEWS.values():
        fn = getattr(ops, v.name)
        assert fn.__name__ == v.name and fn.__doc__ == v.doc
        assert str(inspect.signature(fn)) == '(device=0)'
        if v.reset is None:
            assert re.search(r"^%s = _counter_fns\('%s'\)\[0\]" % (v.name, v.name), text, flags=re.M), v.name
            continue
        assert re.search(r"^%s, %s = _counter_fns\('%s'\)$" % (v.name, v.reset, v.name), text, flags=re.M), v.name
        rs = getattr(ops, v.reset)
        assert rs.__name__ == v.reset and str(inspect.signature(rs)) == '(device=0)'
    assert text.count('c_ulonglong') == 1                                   # the one reader
    assert not re.search(r'len\(\w*_KEYS\)\s*\+', text)
    # the Python-side counters are not part of the table
    assert 'prep_counts' not in _counters.VIEWS and callable(ops.prep_counts) and callable(ops.reset_prep_counts)


class _RampLib(object):
    """Stands for a handle's library: a getter fills out[i] = base + i and logs (name, n or None), a reset logs its name."""

    def __init__(self, base, log):
        self.base, self.log = base, log

    def __getattr__(self, name):
        if name.startswith('asr_reset_'):
            def reset(h):
                self.log.append((name, None))
                return 0
            return reset

        def get(h, out, *n):
            assert len(n) <= 1 and all(v == len(out) for v in n), (name, n, len(out))
            self.log.append((name, n[0] if n else None))
            for i in range(len(out)):
                out[i] = self.base + i
            return 0
        return get


class _FakeHandle(object):
    def __init__(self, base, log):
        self.h, self.lib = None, _RampLib(base, log)

    def check(self, rc, what):
        assert rc == 0, what


def test_key_order_and_stand_ins(monkeypatch):
    log = []
    handles = [_FakeHandle(100, log), _FakeHandle(1000, log)]
    monkeypatch.setattr(ops, '_device_handles', lambda device: handles)
    got = wn_ops.install(monkeypatch)
    assert got is ops
    # the patched names still win: models look them up on ops at call time
    for name, fn in wn_ops.STAND_INS.items():
        assert getattr(ops, name) is fn
    assert ops.weight_noise_counts() == dict(calls=0, elements=0, vec_calls=0) and log == []
    for v in _counters.VIEWS.values():
        if v.name in wn_ops.STAND_INS:
            continue
        fam = _counters.FAMILIES[v.family]
        del log[:]
        d = getattr(ops, v.name)()
        assert list(d.keys()) == list(v.keys), v.name                       # table order
        assert list(d.values()) == [1100 + 2 * (v.offset + i) for i in range(len(v.keys))], v.name
        n = len(fam.keys) if fam.sized else None
        assert log == [(fam.getter, n)] * 2, (v.name, log)                  # one native call per handle
        if v.reset is not None:
            del log[:]
            assert getattr(ops, v.reset)(0) is None
            assert log == [(fam.reset, None)] * 2


def test_unknown_view_is_an_error():
    with pytest.raises(KeyError):
        ops._counter_fns('no_such_counts')
