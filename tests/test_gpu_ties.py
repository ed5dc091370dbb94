"""The near-tie counter on the device against the oracle twin's restatement of its definition (oracle/ghmm_twin.cc: twin_near_ties;
DESIGN.md 6 "near-ties") and against the emulator, so that a failure says which side moved.  tests/test_emu_ties.py describes the
comparison, the two thresholds, the inputs and the shapes they are there for (asserted there from the twin's output: the records are
the same, helpers.ties_records).  Here:

- kTrellis<BLK, MODE, true> + kBacktrace under human (block 8), caenorhabditis (block 4) and human at AUGX_BLK=2, whole and -- the record of
  helpers.trellis_edge_long, AUGX_SEG_LEN=77000 -- in segments; kDense<BLK, 0, true> + kDenseBacktrace under human --UTR=on at block 4 and 2,
  fly --UTR=on, the model with two intergenic states and maize;
- every batch in the given and in the reversed order of its records, each decoded twice;
- for every piece: status, score, path (and, on the first decode, every cell) equal the twin's; the flag of every live chain cell
  (Batch.prep: bpChain / bpD as the decode left them) equals the twin's; the bytes equal the emulator's; the count of the piece
  (Batch.near_ties) equals the twin's and the emulator's and is 0 for a piece whose decode fails;
- the sums (cells, pieces) of augx_decoder_near_ties: every fetch of the paths of a batch (Batch.paths) adds the counts of its pieces of
  status 0 and the number of them with at least one -- "the sum over the paths fetched so far" (include/augx.h), so a second fetch of the
  same batch adds them a second time; reading the per-piece counts or the flags adds nothing.

Exact mode is off (the fixture below) as in tests/test_gpu_dense.py: no replay of the reference's caches runs, none revalues a candidate
of the path (memoVitDiffs == 0); test_gpu_ties_exact_mode_two_classes is the piece with two GC classes in exact mode."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *

_emu_want = {}


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")  # (the trellis kernels keep their cells only on request)
    yield
    emu_set_near_tie_eps(None)


def _model(monkeypatch, cfg, blk):
    if blk is None:
        monkeypatch.delenv("AUGX_BLK", raising=False)
    else:
        monkeypatch.setenv("AUGX_BLK", blk)
    species, opts = TIES_CFGS[cfg]
    return ax.Model(config_path(), species, **opts)


def _emulator(m, cfg, blk, recs, eps, tag=None):
    """(counts, [flag bytes]) of the emulator for the batch recs at threshold eps, computed once (the caller has set AUGX_BLK and the
    switches of the decode, which the emulator follows)"""
    key = (tag or cfg, blk, eps, tuple(n for n, _ in recs), os.environ.get("AUGX_EXACT_MULTICLASS"), os.environ.get("AUGX_SEG_LEN"), os.environ.get("AUGX_SEG_CHECK_TILES"))
    if key not in _emu_want:
        assert emu_set_near_tie_eps(eps) == 0
        emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, prep=True)
        which = "bpD" if ties_family(cfg) else "bpChain"
        _emu_want[key] = (emu_near_ties(len(recs)), [emu_prep(i, which) for i in range(len(recs))])
    return _emu_want[key]


def check_device(m, cfg, blk, recs, eps, tag=None, orders=2):
    """decode recs on the device at threshold eps -- in the given and in the reversed order, each batch twice -- and compare every piece
    with the twin and the emulator, and the decoder's sums with what the fetches must have added; returns the twins"""
    S, fam = m.n_states, ties_family(cfg)
    chain = twin_chain_states(m.tables_ptr, S)
    which = "bpD" if fam else "bpChain"
    twins = [ties_twin(m, cfg, seq, tag=tag) for _, seq in recs]
    ecount, ebytes = _emulator(m, cfg, blk, recs, eps, tag)
    d = ax.Decoder(m, 0)
    d.count_near_ties(True)
    d.set_near_tie_eps(eps)
    want_sum = [0, 0]
    idx = list(range(len(recs)))
    for order in (idx, idx[::-1])[:orders]:
        b = ax.Batch(d, [recs[i][1] for i in order])
        for turn in range(2):
            b.decode()
            assert d.near_ties() == tuple(want_sum)  # (a decode alone adds nothing)
            res = b.paths()
            counts = b.near_ties()
            for k, i in enumerate(order):
                (name, seq), T, r = recs[i], twins[i], res[k]
                assert r.status == T.rc, (name, turn, r.status, T.rc)
                if T.rc == 0:
                    assert r.ln_viterbi == T.lnv and r.states == T.path, (name, turn)
                if turn == 0 and order is idx and set(seq.upper()) != {"N"}:
                    assert np.array_equal(b.cells(k), T.V), name
                raw = b.prep(k, which)
                flags = chain_flags_of(raw, chain, S, dense=bool(fam))
                assert ties_first_diff(flags, T, eps) is None, (name, turn, eps, ties_first_diff(flags, T, eps))
                # the bytes themselves against the emulator's: base 0 of a piece holds nothing
                assert np.array_equal(np.asarray(raw).reshape(len(seq), -1)[1:], np.asarray(ebytes[i]).reshape(len(seq), -1)[1:]), (name, turn)
                want = T.counts(eps)[0] if T.rc == 0 else 0
                assert counts[k] == want == ecount[i], (name, turn, eps, counts[k], want, ecount[i])
                want_sum[0] += want
                want_sum[1] += want > 0
            assert d.near_ties() == tuple(want_sum), (turn, d.near_ties(), want_sum)
            assert b.near_ties() == counts and d.near_ties() == tuple(want_sum)  # (reading the counts adds nothing)
        b.close()
    d.close()
    return twins


@pytest.mark.parametrize("which", ["product", "large"])
@pytest.mark.parametrize("cfg,blk", TIES_TRELLIS + TIES_DENSE)
def test_gpu_ties_flags_counts_and_sums_equal_the_twin(monkeypatch, cfg, blk, which):
    m = _model(monkeypatch, cfg, blk)
    eps = TIES_PRODUCT_EPS if which == "product" else TIES_EPS[cfg]
    recs = ties_records(cfg)
    twins = check_device(m, cfg, blk, recs, eps)
    by = {name: T for (name, _), T in zip(recs, twins)}
    if which == "large":
        for name in TIES_ON_PATH[ties_family(cfg)]:
            assert by[name].rc == 0 and 0.01 <= ties_share(by[name], eps) <= 0.5, (name, ties_share(by[name], eps))
        assert sum(T.counts(eps)[0] for T in twins if T.rc == 0) > 100
    if cfg == "human_atleastone":  # (no room for a gene, no path: such a piece adds nothing to the sums)
        assert sum(1 for T in twins if T.rc != 0) >= 3


def test_gpu_ties_a_second_fetch_adds_again_and_the_setter_refuses(monkeypatch):
    """include/augx.h: augx_decoder_near_ties is the sum over the paths FETCHED so far; augx_decoder_set_near_tie_eps applies to the batches
    created afterwards and refuses a threshold that is not finite and positive"""
    m = _model(monkeypatch, "human", None)
    by = dict(golden_inputs())
    seqs = [by["HS04636"], by["short100"], by["softmask_all"]]
    twins = [ties_twin(m, "human", s) for s in seqs]
    eps = TIES_EPS["human"]
    want = [T.counts(eps)[0] for T in twins]
    assert all(T.rc == 0 for T in twins) and min(want) > 0
    d = ax.Decoder(m, 0)
    d.count_near_ties(True)
    b0 = ax.Batch(d, seqs)  # (created before the setter: the product's threshold)
    d.set_near_tie_eps(eps)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ax.AugxError):
            d.set_near_tie_eps(bad)
    b = ax.Batch(d, seqs)
    b.decode()
    assert d.near_ties() == (0, 0)
    b.paths()
    assert d.near_ties() == (sum(want), 3) and b.near_ties() == want
    b.paths()
    assert d.near_ties() == (2 * sum(want), 6)
    b0.decode()
    b0.paths()
    assert b0.near_ties() == [0, 0, 0] and d.near_ties() == (2 * sum(want), 6)
    d.count_near_ties(False)
    b1 = ax.Batch(d, seqs[:1])  # (a batch that does not count has no counts to hand out)
    b1.decode()
    with pytest.raises(ax.AugxError):
        b1.near_ties()
    for x in (b, b0, b1):
        x.close()
    d.close()


def test_gpu_ties_runner_up_that_shares_the_winners_end(monkeypatch):
    """human --UTR=on at TIES_EPS_SHARED_END (tests/test_emu_ties.py: the same test): the winner is excluded by end and ancestor"""
    m = _model(monkeypatch, "human_utr", "4")
    by = dict(golden_inputs())
    eps = TIES_EPS_SHARED_END
    twins = check_device(m, "human_utr", "4", [(k, by[k]) for k in ("withN", "HS04636")], eps)
    assert all(0.01 <= ties_share(T, eps) <= 0.5 for T in twins)


def test_gpu_ties_soak_case_5010(monkeypatch):
    """the one known near tie at the product's threshold, an exact tie: base 12976 of the stretch, intergenic state, inside a run (trellis
    kernels); the same cell as the entry cell of its run under the model with two intergenic states (dense kernels; tests/test_emu_ties.py)"""
    import soak_cli
    monkeypatch.delenv("AUGX_BLK", raising=False)
    _, g = soak_cli.real_dna()
    recs, _, _ = soak_cli.make_case(5010, g)
    seq = recs[1][1][:50000].upper()
    eps = TIES_PRODUCT_EPS
    for cfg, opts, s, want in (("human", {"softmasking": "0"}, seq, (12976, 0, 1, 0.0, 0.0)),
                               ("human_atleastone", {"softmasking": "0", "genemodel": "atleastone", "sample": "0"}, seq[8000:16000], (4976, 47, 0, 0.0, 0.0))):
        m = ax.Model(config_path(), "human", **opts)
        T, = check_device(m, cfg, None, [("5010", s)], eps, tag=cfg + ", no soft-masking")
        assert [it for it in T.items if it[3] < eps or it[4] < eps] == [want] and T.counts(eps) == (1, 1)


def test_gpu_ties_exact_mode_two_classes(monkeypatch):
    """multigc_two in exact mode: the replay of the reference's snippet cache patches candidate terms and the trellis runs a second time,
    which rewrites the flags; against the twin with its restatement of the cache"""
    monkeypatch.delenv("AUGX_BLK", raising=False)
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "1")
    m = ax.Model(config_path(), "human")
    seq = dict(golden_inputs())["multigc_two"]
    for eps in (TIES_PRODUCT_EPS, TIES_EPS["human"]):
        T, = check_device(m, "human", None, [("multigc_two", seq)], eps)
    assert len(emu_replay_log()[1].get(0, {})) > 0 and 0.01 <= ties_share(T, TIES_EPS["human"]) <= 0.5


@pytest.mark.parametrize("cfg,blk", TIES_TRELLIS)
@pytest.mark.parametrize("env", [{"AUGX_SEG_LEN": "77000"}, {"AUGX_SEG_LEN": "77000", "AUGX_SEG_CHECK_TILES": "100000"}], ids=["check", "nocheck"])
def test_gpu_ties_segments(monkeypatch, env, cfg, blk):
    """the record of helpers.trellis_edge_long in five segments: the twin, which knows no segments, has flagged cells in the tiles that a
    fix-up rewrote, in those a continuation rewrote and (unreachable check length) in those left to the last pass; check_device compares
    every flag of the piece"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(monkeypatch, cfg, blk)
    eps = TIES_EPS[cfg]
    seq = trellis_edge_long()
    T, = check_device(m, cfg, blk, [("long", seq)], eps)
    d = ax.Decoder(m, 0)
    b = ax.Batch(d, [seq])
    b.decode()
    plan = b.plan()
    b.close()
    d.close()
    assert len(plan["segs"]) == 5
    ties_assert_rewritten_tiles(T, eps, [(k, t0, t1, stop, stop2) for (piece, k, t0, t1, tlim), stop, stop2 in zip(plan["segs"], plan["seg_stop"], plan["seg_stop2"])],
                                "AUGX_SEG_CHECK_TILES" in env)
    assert 0.01 <= ties_share(T, eps) <= 0.5
