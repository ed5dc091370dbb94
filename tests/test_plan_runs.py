"""The plan of the trellis passes (layout.h: planSegments) through its read-only query (augx_plan_segments; host only, no device):
runs of segments over the whole device for the bench shape, the invariants of any plan on seeded random batches, and the cases in
which the plan must stay what it was: many short pieces, one piece, a segment length given by AUGX_SEG_LEN."""
import random

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *

WAVE = 64


@pytest.fixture(scope="module")
def human():
    return ax.Model(config_path(), "human")


def _tiles(lens):
    return [(n + WAVE - 1) // WAVE for n in lens]


def _runs(P):
    r0 = P["run_seg0"]
    return [list(range(r0[i], r0[i + 1])) for i in range(P["n_runs"])]


def _check_plan(P, lens, slots):
    """what holds for every plan: the segments of a piece tile it in order, none is shorter than its rule, tlim is t1 - checkTiles - 2;
    the runs are contiguous, cover every segment, are no more than the slots, and none holds two segments of one piece"""
    segs, ck = P["segs"], P["check_tiles"]
    tiles = _tiles(lens)
    assert ck > 0
    q = 0
    for p, nt in enumerate(tiles):
        k, t = 0, 0
        while q < len(segs) and segs[q][0] == p:
            piece, kk, t0, t1, tlim = (int(x) for x in segs[q])
            assert kk == k and t0 == t and t1 > t0 and tlim == t1 - ck - 2, (p, q)
            k, t, q = k + 1, t1, q + 1
        assert k >= 1 and t == nt, p
        if k > 1:  # a cut piece: the first segment holds the look-back of the next fix-up, every other one a fix-up of its own as well
            first = q - k
            assert segs[first][3] - segs[first][2] >= ck + 2, p
            for s in range(first + 1, q):
                assert segs[s][3] - segs[s][2] >= 5 * ck, (p, s)
    assert q == len(segs)
    if P["n_runs"] == 0:
        assert len(P["run_seg0"]) == 0
        return
    r0 = P["run_seg0"]
    assert 1 <= P["n_runs"] <= slots and len(r0) == P["n_runs"] + 1
    assert r0[0] == 0 and r0[-1] == len(segs) and all(r0[i] < r0[i + 1] for i in range(P["n_runs"]))
    for run in _runs(P):
        pieces = [int(segs[s][0]) for s in run]
        assert len(set(pieces)) == len(pieces), run
    assert len(segs) > len(lens)  # (runs are made only where a piece is cut)


def test_bench_shape_takes_runs_over_the_whole_device(human):
    lens = [1000000] * 100
    P = ax.plan_segments(human, lens, 256)
    _check_plan(P, lens, 256)
    segs = P["segs"]
    assert 0 < P["n_runs"] <= 256
    assert int((segs[:, 1] > 0).sum()) <= 255  # one round of fix-ups
    length = segs[:, 3] - segs[:, 2]
    longest = max(int(length[r].sum()) for r in _runs(P))
    total = sum(_tiles(lens))
    print("bench shape: %d segments, %d runs, %d fix-ups, longest run %d tiles = %.4f x mean" % (len(segs), P["n_runs"], int((segs[:, 1] > 0).sum()), longest, longest * 256 / total))
    assert longest <= 1.02 * total / 256
    assert P["est_tiles"] < P["est_per_piece"]


@pytest.mark.parametrize("seed", range(50))
def test_plan_invariants_on_random_batches(human, seed):
    rng = random.Random(4000 + seed)
    n = rng.choice([1, 2, 3, 5, 8, 20, 60, 100, 300]) if seed % 3 else rng.randint(1, 300)
    # (lengths spread over the decades: batches of short pieces, of long ones, and mixes)
    lens = [int(5000 * (560 ** rng.random())) for _ in range(n)]
    assert all(5000 <= x <= 2800000 for x in lens)
    slots = (1, 32, 256)[seed % 3]
    P = ax.plan_segments(human, lens, slots)
    _check_plan(P, lens, slots)
    assert 0 < P["est_tiles"] <= P["est_per_piece"]


def test_many_short_pieces_are_not_cut(human):
    lens = [100000] * 1000
    P = ax.plan_segments(human, lens, 256)
    _check_plan(P, lens, 256)
    assert len(P["segs"]) == 1000 and P["n_runs"] == 0


def test_one_piece_is_planned_no_worse_than_piece_by_piece(human):
    lens = [1000000]
    P = ax.plan_segments(human, lens, 256)
    _check_plan(P, lens, 256)
    assert len(P["segs"]) > 1
    assert 0 < P["est_tiles"] <= P["est_per_piece"]  # (est_per_piece: the best of the equal cuts of the piece, by the same estimate)


@pytest.mark.parametrize("seg_len", [100000, 77000])
def test_given_segment_length_cuts_every_piece_equally(human, monkeypatch, seg_len):
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len))
    lens = [1000000, 390000, 90000, 230001, 2800000, 77000, 154000]
    P = ax.plan_segments(human, lens, 256)
    _check_plan(P, lens, 256)
    assert P["n_runs"] == 0
    st, min_seg = (seg_len + WAVE - 1) // WAVE, 5 * P["check_tiles"]
    want = []
    for p, nt in enumerate(_tiles(lens)):
        kp = max(1, (nt + st // 2) // st)  # the nearest count, no segment shorter than min_seg
        while kp > 1 and nt // kp < min_seg:
            kp -= 1
        want += [(p, k, nt * k // kp, nt * (k + 1) // kp) for k in range(kp)]
    assert len(want) <= 256  # (no more segments than slots: no piece gets one more to fill a round)
    assert [tuple(int(x) for x in s[:4]) for s in P["segs"]] == want
    assert len(want) > len(lens)
