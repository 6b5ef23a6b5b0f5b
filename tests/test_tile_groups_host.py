"""CPU: the plan of the cluster recurrences' tile groups (asr_cluster_tile_groups, csrc/cluster_host.hip) -- pure integer
arithmetic behind the C ABI, no GPU.  A launch of G workgroups per cluster over m tiles needs 8 G ceil(m ndir / 8)
co-resident workgroups; a batch that needs more than the budget runs as consecutive launches over tile ranges."""
import ctypes as C
import itertools

import pytest

GS = (2, 4, 5, 8, 10, 16)
NDIRS = (1, 2)
BUDGETS = (64, 128, 256, 304)
MAX_TILES = 40


def _grid(G, clusters):
    return 8 * G * ((clusters + 7) // 8)


@pytest.fixture(scope='module')
def plan():
    from tensorflow_end2end_speech_recognition_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        from tensorflow_end2end_speech_recognition_amd.build import build
        build(verbose=False)
    lib = _lib.load()

    def call(G, ndir, tiles, budget):
        first, cnt = (C.c_int * tiles)(), (C.c_int * tiles)()
        n = lib.asr_cluster_tile_groups(G, ndir, tiles, budget, first, cnt, tiles)
        assert 0 <= n <= tiles, (G, ndir, tiles, budget, n)
        return [(first[i], cnt[i]) for i in range(n)]
    return call


def _fewest_groups(G, ndir, tiles, budget):
    """Brute force: the fewest consecutive groups that cover `tiles` tiles, each within the budget (None: impossible).
    best[t] = fewest groups for the first t tiles, over every size of the last group."""
    fits = [m for m in range(1, tiles + 1) if _grid(G, m * ndir) <= budget]
    best = [0] + [None] * tiles
    for t in range(1, tiles + 1):
        cands = [best[t - m] + 1 for m in fits if m <= t and best[t - m] is not None]
        best[t] = min(cands) if cands else None
    return best[tiles]


@pytest.mark.parametrize('G,ndir,budget', list(itertools.product(GS, NDIRS, BUDGETS)))
def test_tile_groups_cover_the_batch_within_the_budget_with_the_fewest_launches(plan, G, ndir, budget):
    for tiles in range(1, MAX_TILES + 1):
        groups = plan(G, ndir, tiles, budget)
        what = (G, ndir, tiles, budget, groups)
        if _grid(G, ndir) > budget:                      # not even one tile fits: no plan, the caller falls back
            assert groups == [], what
            continue
        assert groups, what
        nxt = 0
        for first, n in groups:                          # consecutive, disjoint, covering [0, tiles)
            assert first == nxt and n >= 1, what
            assert _grid(G, n * ndir) <= budget, what    # every group is a legal launch on its own
            nxt = first + n
        assert nxt == tiles, what
        assert (len(groups) == 1) == (_grid(G, tiles * ndir) <= budget), what
        assert len(groups) == _fewest_groups(G, ndir, tiles, budget), what


def test_tile_groups_examples_and_bad_arguments(plan):
    from tensorflow_end2end_speech_recognition_amd import _lib, ops
    assert plan(8, 2, 5, 64) == [(0, 4), (4, 1)]          # B = 80 on a budget of 64: a full group and a partial one
    assert plan(8, 2, 16, 256) == [(0, 16)]               # B = 256 at H = 256 fills a 256-CU chip
    assert plan(8, 2, 17, 256) == [(0, 16), (16, 1)]      # B = 272: one tile more than the chip holds
    assert plan(16, 2, 17, 256) == [(0, 8), (8, 8), (16, 1)]
    assert plan(16, 1, 3, 64) == [] and plan(10, 2, 1, 64) == []
    assert ops.cluster_tile_groups(8, 2, 5, 64) == [(0, 4), (4, 1)]
    lib = _lib.load()
    for bad in ((0, 2, 4, 64), (8, 0, 4, 64), (8, 3, 4, 64), (8, 2, 0, 64), (8, 2, 4, 0), (8, 2, 4, -5)):
        assert lib.asr_cluster_tile_groups(*bad, None, None, 0) < 0, bad
    assert lib.asr_cluster_tile_groups(8, 2, 5, 64, None, None, 0) == 2      # count only
