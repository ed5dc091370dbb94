"""The back-trace kernel (kernels.h: backtracePiece) on runs of the single-base chain states of every length around the edges of its
rounds of loads.  A chain run is walked a round of bases at a time -- the back pointers of the whole round are loaded before the first
is tested --, so what can go wrong is a run that ends on, one before or one after the last base of a round, in the first or the last
lane, at base 1 of the piece (the walk must not read before the piece's slots), and a run that begins and ends inside a piece.  Human
model, one batch, with and without the count of near ties (the two forms of the round), decoded twice; for every record status, score
and state path must equal the oracle twin's.

- Prefixes of the golden record softmask_all of n = 1..300 bases and n = 256 k + d, k = 1..31, d in {-1, 0, 1, 2}: under the human model
  each decodes to ONE intergenic run of n - 1 bases (asserted from the twin's path, so that a record that stops having this shape
  cannot hide a failure).  Every multiple of 256 up to 7 936 is there: the test does not know the size of a round.
- Records of N of the same lengths up to 256 * 8 + 2: the trellis jumps over runs of N and writes their chain bytes itself.
- The golden records with long runs in the geometric intron states and runs that begin and end inside the piece."""
import os

import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *

EDGE_LENS = sorted(set(range(1, 301)) | {256 * k + d for k in range(1, 32) for d in (-1, 0, 1, 2)})
N_LENS = [n for n in EDGE_LENS if n <= 256 * 8 + 2]
GOLDEN_RUNS = {"rand60k": (0, 28351), "withN": (12, 13656), "softmask_rand": (45, 13421), "multigc_levels": (22, 7412), "HS04636": None}


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """as in test_gpu_parity.py: the first pass on its own against the twin without its snippet cache"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")


@pytest.fixture(scope="module")
def cases():
    """(model, [(name, sequence)], [(ln Viterbi, path) of the twin]): computed once for both builds"""
    saved = os.environ.get("AUGX_EXACT_MULTICLASS")
    os.environ["AUGX_EXACT_MULTICLASS"] = "0"  # (twin_decode follows the switch; the autouse fixture is per test)
    try:
        m = ax.Model(config_path(), "human")
        by = dict(golden_inputs())
        src = by["softmask_all"]
        assert len(src) >= EDGE_LENS[-1]
        recs = [("softmask_all[:%d]" % n, src[:n]) for n in EDGE_LENS] + [("N*%d" % n, "N" * n) for n in N_LENS]
        n_runs = len(recs)
        recs += [(name, by[name]) for name in GOLDEN_RUNS]
        want = []
        for name, seq in recs:
            rc, lnv, path, _, _ = twin_decode(m.tables_ptr, seq, m.n_states)
            assert rc == 0, name
            want.append((lnv, path))
    finally:
        if saved is None:
            os.environ.pop("AUGX_EXACT_MULTICLASS", None)
        else:
            os.environ["AUGX_EXACT_MULTICLASS"] = saved
    # the shapes the records are there for, from the twin's own paths
    for (name, seq), (_, path) in zip(recs[:n_runs], want[:n_runs]):
        assert path == ([(1, len(seq) - 1, 0, 0)] if len(seq) > 1 else []), name
    longest = 4096  # (two rounds of loads; the runs counted are those of the intron states, the twin's 12, 17, 22, 40 and 45)
    n_long = 0
    for (name, _), (_, path) in zip(recs[n_runs:], want[n_runs:]):
        runs = [(s, e - b + 1) for b, e, s, _ in path]
        if GOLDEN_RUNS[name] is not None:
            assert GOLDEN_RUNS[name] in runs, (name, sorted(runs, key=lambda r: -r[1])[:4])
        n_long += sum(1 for s, ln in runs if s != 0 and ln > longest)
    assert n_long >= 3
    return m, recs, want


@pytest.mark.parametrize("ties", [False, True])
def test_gpu_backtrace_runs_at_the_round_edges(cases, ties):
    m, recs, want = cases
    d = ax.Decoder(m, 0)
    d.count_near_ties(ties)
    b = ax.Batch(d, [s for _, s in recs])
    for turn in ("first decode", "second decode"):
        b.decode()
        res = b.paths()
        assert len(res) == len(recs)
        for (name, _), r, (lnv, path) in zip(recs, res, want):
            assert r.status == 0, (turn, name, r.status)
            assert r.ln_viterbi == lnv, (turn, name, r.ln_viterbi, lnv)
            assert r.states == path, (turn, name)
    b.close()
    d.close()
