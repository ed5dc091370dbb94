"""The near-tie counter (include/augx.h: augx_decoder_count_near_ties) in the lane-loop emulator against the oracle twin's restatement
of its definition (oracle/ghmm_twin.cc: twin_near_ties; DESIGN.md 6 "near-ties").  CPU only; tests/test_gpu_ties.py makes the same
comparisons on the device.

What is compared, for every piece, exactly (every value is a sum of multiples of 2^-31, the cells are bit-identical to the twin's):
 1. the flag of every live chain cell -- bit 7 of the bpChain bytes of the trellis kernels, bit 6 of the bpD bytes of the dense kernels,
    as the decode left them (emu_prep) -- and that a cell holds a back pointer exactly where the twin's cell is live;
 2. the count of the piece (emu_near_ties), which is 0 for a piece whose decode fails;
 3. status, score, path and cells, as everywhere.
The emulator has no decoder object: the sums (cells, pieces) of augx_decoder_near_ties are checked on the device.

Two thresholds (emu_set_near_tie_eps, the emulator's augx_decoder_set_near_tie_eps): the product's 2e-7, at which real inputs have no near
tie but the stretch of soak case 5010, and TIES_EPS of the configuration, at which between 1 % and 50 % of the chain cells of the paths of
the records of TIES_ON_PATH are flagged (asserted from the twin's margins).  The shapes the inputs are there for -- flagged and unflagged
cells at the edges of the rounds of loads of the back-trace, in the first and the last lane, at base 1 and at the last base, runs that
reach base 1, flagged and unflagged entry cells, every chain slot, every kind of variable-length element, an exact tie of one -- are
asserted from the twin's output (helpers.ties_conditions), so that a fixture that loses a shape cannot hide a failure.

With AUGX_EXACT_MULTICLASS=0 (the fixture below) no replay of the reference's caches runs, so none revalues a candidate of the path
(memoVitDiffs == 0); test_emu_ties_exact_mode_two_classes is the piece with two GC classes in exact mode, whose second trellis run
rewrites the flags."""
import os
import re

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *



@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """as in test_emu.py: the first pass on its own, the twin's restatement of the snippet cache off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")
    yield
    emu_set_near_tie_eps(None)  # (the emulator's threshold is a setting of the process: back to the product's)


def _model(monkeypatch, cfg, blk):
    if blk is None:
        monkeypatch.delenv("AUGX_BLK", raising=False)
    else:
        monkeypatch.setenv("AUGX_BLK", blk)
    species, opts = TIES_CFGS[cfg]
    return ax.Model(config_path(), species, **opts)


def check_emulator(m, cfg, recs, eps, lib=None, init_kind=0, term_kind=0, tag=None):
    """decode recs in one batch on the emulator at threshold eps and compare every piece with the twin; returns the twins.  tag: the
    model when it is not the one of TIES_CFGS[cfg] (the twin's results are kept by it)"""
    S, fam = m.n_states, ties_family(cfg)
    chain = twin_chain_states(m.tables_ptr, S)
    assert emu_set_near_tie_eps(eps, lib) == 0
    res = emu_decode(m.tables_ptr, [s for _, s in recs], S, cells=True, prep=True, lib=lib, init_kind=init_kind, term_kind=term_kind)
    counts = emu_near_ties(len(recs), lib)
    if os.environ.get("AUGX_EXACT_MULTICLASS") == "0":  # (no replay ran: none revalued a candidate of a path, none rebuilt a term)
        cnt, patched, _ = emu_replay_log(lib)
        assert cnt["vit_diffs"] == 0 and cnt["calls"] == 0 and not patched, cnt
    twins = []
    for i, ((name, seq), (st, lnv, path, V, _)) in enumerate(zip(recs, res)):
        T = ties_twin(m, cfg, seq, init_kind, term_kind, tag)
        twins.append(T)
        assert st == T.rc or (st == ax.AUGX_E_NOPATH and T.rc != 0), (name, st, T.rc)
        if T.rc == 0:
            assert lnv == T.lnv and path == [(b, e, s) for b, e, s, _ in T.path], name
        if set(seq.upper()) != {"N"}:
            assert np.array_equal(V, T.V), name
        flags = chain_flags_of(emu_prep(i, "bpD" if fam else "bpChain", lib=lib), chain, S, dense=bool(fam))
        assert ties_first_diff(flags, T, eps) is None, (name, eps, ties_first_diff(flags, T, eps))
        assert counts[i] == (T.counts(eps)[0] if T.rc == 0 else 0), (name, eps, counts[i], T.counts(eps))
        # what the kernels flag is a subset of the full definition (the true runner-up over all ancestors, no index guard)
        assert np.all((T.flags(eps) != 1) | (T.flags(eps, full=True) == 1)), name
        assert T.counts(eps)[0] <= T.counts(eps)[1], name
    return twins


@pytest.mark.parametrize("which", ["product", "large"])
@pytest.mark.parametrize("cfg,blk", TIES_TRELLIS + TIES_DENSE)
def test_emu_ties_flags_and_counts_equal_the_twin(monkeypatch, cfg, blk, which):
    m = _model(monkeypatch, cfg, blk)
    assert emu_block_size(m.tables_ptr) == int(blk or {"caenorhabditis": 4}.get(cfg, 8))
    eps = TIES_PRODUCT_EPS if which == "product" else TIES_EPS[cfg]
    recs = ties_records(cfg)
    twins = check_emulator(m, cfg, recs, eps)
    by = {name: T for (name, _), T in zip(recs, twins)}
    if which == "product":
        # these inputs have no near tie on their paths at the product's threshold, under the full definition either; the only cells
        # flagged are exact ties off the path (margin 0: the repeats that begin with ACGT x 500 have one under the human model with UTR states)
        assert all(T.counts(eps) == (0, 0) for T in twins)
        assert all(float(np.nansum(np.where(T.flags(eps, full=True) == 1, T.margin_full, 0.0))) == 0.0 for T in twins)
    else:
        for name in TIES_ON_PATH[ties_family(cfg)]:
            assert by[name].rc == 0 and 0.01 <= ties_share(by[name], eps) <= 0.5, (name, ties_share(by[name], eps))
    if cfg == "human_atleastone":  # (two intergenic states: no room for a gene, no path; such a piece counts nothing)
        assert sum(1 for T in twins if T.rc != 0) >= 3


@pytest.mark.parametrize("cfg", [c for c, b in TIES_TRELLIS + TIES_DENSE if b != "2"])
def test_emu_ties_inputs_have_the_shapes(monkeypatch, cfg):
    """the conditions on the inputs, from the twin's path and margins alone (ties_conditions says what each name means)"""
    m = _model(monkeypatch, cfg, None)
    S, fam = m.n_states, ties_family(cfg)
    eps = TIES_EPS[cfg]
    R = emu_trellis_windows()["BT_ROUND_DENSE" if fam else "BT_ROUND"]
    assert R == (256 if fam else 2048)  # (TIES_FOUND was searched for these rounds: a new size of the round needs a new search)
    chain = twin_chain_states(m.tables_ptr, S)
    recs = ties_records(cfg)
    got, got_product, lone = set(), set(), {}
    cls, kind = twin_tie_classes(m.tables_ptr, S)
    for name, seq in recs:
        T = ties_twin(m, cfg, seq)
        for b, s, rule, mk, _ in T.items:
            if rule == 2:
                lone[kind[s]] = lone.get(kind[s], True) and mk == float("inf")
        got |= ties_conditions(T, eps, R, chain, kind, dense=bool(fam))
        got_product |= ties_conditions(T, TIES_PRODUCT_EPS, R, chain, kind, dense=bool(fam))
    assert TIES_CORE | TIES_SHAPES[cfg] <= got, sorted((TIES_CORE | TIES_SHAPES[cfg]) - got)
    assert {"entry_noflag", "run_to_base1", "entry_noflag_d0", "entry_noflag_dR-1"} <= got_product
    if cfg in TIES_ONE_ANCESTOR_PER_END:
        # no cell of a variable-length state on any path has two live candidates of one predecessor end: a runner-up that shares the winner's
        # end and differs in the ancestor cannot exist under this model, and excluding the winner by its end alone is the same computation
        assert "var_shared_end_rec" not in got and "var_same_rec" not in got
    # every chain slot holds a flagged cell, and the path of some record a flagged cell of it; every kind of variable-length state is
    # counted on some path -- but for the slots and kinds helpers.py lists with the reason
    no_slot = TIES_NO_SLOT.get(cfg, set())
    assert {"cells_slot%d" % c for c in range(len(chain)) if not (cfg == "human_atleastone" and c == 0)} <= got
    assert {c for c in range(len(chain)) if "slot%d" % c not in got} == no_slot
    counted = {kind[int(c[3:])] for c in got if re.fullmatch(r"var\d+", c)}
    assert {kind[s] for s in range(S) if cls[s] == 2} - counted == TIES_KINDS_UNCOUNTED[cfg], sorted({kind[s] for s in range(S) if cls[s] == 2} - counted)
    if cfg in TIES_ONE_ANCESTOR_PER_END:
        # (why reverse single and reverse terminal exons are never counted under the 47-state models: the paths hold reverse terminal
        # exons, and the twin gives every such element no margin at all -- its cell has one candidate)
        never = {k for k, v in lone.items() if v}
        assert K_RTERMINAL in never and never <= {K_RSINGLE, K_RTERMINAL} and not ({K_RSINGLE, K_RTERMINAL} & set(lone)) - never, (never, sorted(lone))


def test_emu_ties_runner_up_that_shares_the_winners_end(monkeypatch):
    """human --UTR=on at TIES_EPS_SHARED_END: withN has a counted UTR exon element whose runner-up shares the winner's predecessor end and
    differs in the ancestor (asserted from the twin's list); the count is the twin's only when pass 1 excludes the winner by end AND
    ancestor"""
    m = _model(monkeypatch, "human_utr", "4")
    by = dict(golden_inputs())
    eps = TIES_EPS_SHARED_END
    recs = [(k, by[k]) for k in ("withN", "HS04636")]
    twins = check_emulator(m, "human_utr", recs, eps)
    _, kind = twin_tie_classes(m.tables_ptr, m.n_states)
    c = ties_conditions(twins[0], eps, emu_trellis_windows()["BT_ROUND_DENSE"], twin_chain_states(m.tables_ptr, m.n_states), kind, dense=True)
    assert {"var_same_utr", "var_chunks_utr"} <= c and all(0.01 <= ties_share(T, eps) <= 0.5 for T in twins)


@pytest.mark.parametrize("cfg,blk", TIES_TRELLIS)
def test_emu_ties_exact_tie_of_two_predecessor_ends(monkeypatch, cfg, blk):
    """An exactly tied variable-length element under the models of the trellis kernels, reached through the model: no DNA found has one
    (DESIGN.md 6), because each predecessor end has one feasible ancestor there and two ends are never bit-equal by chance.  The twin
    names the first counted coding exon of the path of HS04636, its margin and the exon length of its runner-up; in a copy of the
    tables that length's entry of the length distribution is raised by the margin -- a multiple of 2^-31 like every term --, and
    winner and runner-up are the same double.  Asserted from the twin on the new tables: the element is on the path with margin 0
    and is NOT counted (the reference decides an exact tie by its own rule, the same in both).  The emulator must give the twin's
    path, cells and count: `best.v != runnerUp` in the trellis back-trace decides it"""
    m = _model(monkeypatch, cfg, blk)
    _, kind = twin_tie_classes(m.tables_ptr, m.n_states)
    eps = TIES_EPS[cfg]
    seq = dict(golden_inputs())["HS04636"]
    T = ties_twin(m, cfg, seq)
    b, s, mk = next((b, s, mk) for b, s, rule, mk, _ in T.items if rule == 2 and 0 < mk < eps and T.cands[(b, s)][3] not in (0, T.cands[(b, s)][4]))
    m2 = BumpedTables(m, kind[s], T.cands[(b, s)][3], mk)
    T2, = check_emulator(m2, cfg, [("HS04636", seq)], eps, tag="%s, length %d of kind %d raised by %r" % (cfg, T.cands[(b, s)][3], kind[s], mk))
    assert [it[2:] for it in T2.items if it[:2] == (b, s)] == [(2, 0.0, 0.0)]
    counted = sum(1 for it in T2.items if it[3] < eps)
    assert T2.counts(eps)[0] == counted - sum(1 for it in T2.items if it[2] == 2 and it[3] == 0.0) < counted


def test_emu_ties_soak_case_5010(monkeypatch):
    """the one known near tie at the product's threshold (tests/test_emu.py: test_emulated_near_tie_counter_flags_the_soak_case): the twin's
    list names it -- an EXACT tie (margin 0) at base 12976 of the stretch in the intergenic state, inside an intergenic run (rule 1) under
    the trellis kernels; cut to bases 8000..16000 under the model with two intergenic states (dense kernels) the same cell, base 4976 of
    state 47, is the entry cell of its run (rule 0).  It is the only flagged cell of the whole matrix, under the full definition too"""
    import soak_cli
    monkeypatch.delenv("AUGX_BLK", raising=False)
    _, g = soak_cli.real_dna()
    recs, _, _ = soak_cli.make_case(5010, g)
    seq = recs[1][1][:50000].upper()
    eps = TIES_PRODUCT_EPS
    for cfg, opts, s, want in (("human", {"softmasking": "0"}, seq, (12976, 0, 1, 0.0, 0.0)),
                               ("human_atleastone", {"softmasking": "0", "genemodel": "atleastone", "sample": "0"}, seq[8000:16000], (4976, 47, 0, 0.0, 0.0))):
        m = ax.Model(config_path(), "human", **opts)
        T, = check_emulator(m, cfg, [("5010", s)], eps, tag=cfg + ", no soft-masking")
        assert [it for it in T.items if it[3] < eps or it[4] < eps] == [want]
        assert T.counts(eps) == (1, 1)
        assert np.argwhere(T.flags(eps, full=True) == 1).tolist() == [[want[0], want[1]]]


def test_emu_ties_exact_mode_two_classes(monkeypatch):
    """multigc_two has two GC classes under the human model: in exact mode the replay of the reference's snippet cache patches candidate
    terms and the trellis runs a second time, which rewrites the flags; with AUGX_EXACT_MULTICLASS=0 it runs once.  Both against the twin
    with and without its restatement of the cache"""
    monkeypatch.delenv("AUGX_BLK", raising=False)
    m = ax.Model(config_path(), "human")
    seq = dict(golden_inputs())["multigc_two"]
    out = []
    for exact in ("0", "1"):
        monkeypatch.setenv("AUGX_EXACT_MULTICLASS", exact)
        for eps in (TIES_PRODUCT_EPS, TIES_EPS["human"]):
            T, = check_emulator(m, "human", [("multigc_two", seq)], eps)
            assert (len(emu_replay_log()[1].get(0, {})) > 0) == (exact == "1")  # (candidate terms rebuilt from the snippet cache)
        out.append(T)
    assert 0.01 <= ties_share(out[0], TIES_EPS["human"]) <= 0.5 and 0.01 <= ties_share(out[1], TIES_EPS["human"]) <= 0.5


@pytest.mark.parametrize("cfg,blk", TIES_TRELLIS)
@pytest.mark.parametrize("env", [{"AUGX_SEG_LEN": "77000"}, {"AUGX_SEG_LEN": "77000", "AUGX_SEG_CHECK_TILES": "100000"}], ids=["check", "nocheck"])
def test_emu_ties_segments(monkeypatch, env, cfg, blk):
    """the record of helpers.trellis_edge_long cut into five segments: the flags of the tiles that a fix-up, a continuation or the last
    pass rewrote are the twin's, which knows no segments (tests/test_emu_trellis.py shows from the emulator's counters that one fix-up
    gives up and is continued, and that with an unreachable check length all four give up, three are continued, one is left to the
    last pass)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = _model(monkeypatch, cfg, blk)
    emu_trellis_coverage_reset()
    T, = check_emulator(m, cfg, [("long", trellis_edge_long())], TIES_EPS[cfg])
    c = emu_trellis_coverage(reset=True)
    assert c["fix_gaveup"] == (4 if "AUGX_SEG_CHECK_TILES" in env else 1) and c["p3_converged"] + c["p3_to_end"] >= 1, c
    segs = emu_seg_stops()
    assert len(segs) == 5
    ties_assert_rewritten_tiles(T, TIES_EPS[cfg], segs, "AUGX_SEG_CHECK_TILES" in env)
    assert 0.01 <= ties_share(T, TIES_EPS[cfg]) <= 0.5


def test_emu_ties_run_of_n_the_trellis_jumps_over(monkeypatch):
    """a run of 3600 N, which the trellis jumps over, writing the chain bytes of the run itself (kernels.h: the jump).  The twin, which
    does no jump, has flagged cells before the run, inside it (its first 600 bases, while the states that were alive before it die) and
    behind it, and its path is one intergenic run through all of it: check_emulator compares every flag and the count"""
    m = _model(monkeypatch, "human", None)
    name, seq = ties_n_jump_record()
    a, b = seq.index("N"), seq.rindex("N") + 1
    eps = TIES_EPS["human"]
    emu_trellis_coverage_reset()
    T, = check_emulator(m, "human", [(name, seq)], eps)
    assert emu_trellis_coverage(reset=True)["jump_restage"] == 1
    f = T.flags(eps)
    assert (f[a - 500:a] == 1).any() and (f[a:b] == 1).any() and (f[b:b + 500] == 1).any()
    assert (f[a:b] == 0).sum() > 10000  # (live, unflagged cells inside the run: what the jump writes)
    assert [p[:3] for p in T.path] == [(1, len(seq) - 1, 0)] and 0.01 <= ties_share(T, eps) <= 0.5


def test_emu_ties_threshold_setter():
    """emu_set_near_tie_eps, as augx_decoder_set_near_tie_eps, refuses what is not finite and positive and keeps the threshold it had"""
    assert emu_set_near_tie_eps(3.5) == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert emu_set_near_tie_eps(bad) == ax.AUGX_E_ARG
    m = ax.Model(config_path(), "human")
    check_emulator(m, "human", [("HS04636", dict(golden_inputs())["HS04636"])], 3.5)
