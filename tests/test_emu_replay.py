"""The replays of the reference's three call-history caches on pieces with several GC classes (device/snipmemo.h: the SnippetProbs cache
of the short introns; device/assmemo.h: the aSSProb memo; dense.h: k1TssReplay), value by value.

Cells, score and path cannot tell whether a rebuilt value is right: a short-intron candidate that is not the arg-max of its cell may
carry any term, and so may an acceptor-site value read by a losing UTR candidate.  Here every rebuilt term and every change of a
site's value is compared with an independent restatement, the log of the oracle twin's own caches (oracle/ghmm_twin.cc:
twin_set_cache_log), as sets: every request the twin's cache answers with mixed content is patched by the replay, with the same
term bit for bit (the terms are sums of multiples of 2^-31 in the same grouping: no tolerance), and nothing else is.

The emulator runs the replay in whole mode (all arrays in host memory) and, with AUGX_EMU_WINDOWED=1, in the windowed mode of the
device library: the plan of the windows and the cut of one window out of the packed arrays are the library's own host functions
(snipmemo.h: planGatherWins, SnippetReplay::cutWindow), the packing of kGatherWindows is restated by a plain loop.
The replays count the paths they take; the inputs (helpers.replay_edge_cases and the multi-class fixtures) reach every one that can be
reached, the others are asserted 0 with the reason.  tests/test_gpu_replay.py runs the same inputs on the device."""
import ctypes
import os

import numpy as np
import pytest

import augustus_amd as ax
from helpers import *

_runs = {}
model, twin_of = replay_model, replay_twin


def fixture_records(cfg):
    """the multi-class fixtures of the other tests that this configuration is run on as well"""
    if cfg not in ("human", "human_utr"):
        return []
    byname = dict(golden_inputs())
    if cfg == "human_utr":  # (the 71-state emulator is slow: the record in which 73 sites change their value during the sweep)
        return [(n, s, 0, 0) for n, s in gc_step_records(1, 7)]
    recs = [("multigc_two", byname["multigc_two"].upper())] + gc_step_records(2, 7)
    return [(n, s, 0, 0) for n, s in recs]


def cases(cfg):
    return replay_edge_cases()[cfg] + fixture_records(cfg)


def emu_run(cfg, windowed=False, env=(), forward=False):
    """(emu_decode's results, replay log) of all cases of a configuration as one batch, computed once per setting"""
    key = (cfg, windowed, tuple(env), forward)
    if key not in _runs:
        m = model(cfg)
        cs = cases(cfg)
        setting = dict(env, AUGX_EMU_WINDOWED="1" if windowed else "0")
        saved = {k: os.environ.get(k) for k in setting}
        os.environ.update(setting)
        try:
            res = emu_decode(m.tables_ptr, [c[1] for c in cs], m.n_states, cells=True, init_kind=[c[2] for c in cs],
                             term_kind=[c[3] for c in cs], forward=forward)
            _runs[key] = (res, emu_replay_log())
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _runs[key]


@pytest.mark.parametrize("windowed", [False, True], ids=["whole", "windowed"])
@pytest.mark.parametrize("cfg", sorted(REPLAY_CFGS))
def test_every_rebuilt_term_is_the_twins_after_the_viterbi_run(cfg, windowed):
    """the replay after the Viterbi run (from the values at the donor sites under the 47-state models, from the dense cells under the
    71-state model): its patches are the twin's mixed requests, and cells, score and path are the twin's"""
    res, (cnt, terms, hist) = emu_run(cfg, windowed)
    n_multi = 0
    for i, case in enumerate(cases(cfg)):
        (rc, lnv, path, V, gc), want, sites, flushes = twin_of(cfg, case)
        assert_terms_equal(terms.get(i, {}), want, (cfg, case[0]))
        n_multi += len(want) > 0
        r = res[i]
        assert r[0] == rc == 0 and r[1] == lnv and r[2] == [(b, e, st) for b, e, st, t in path], case[0]
        assert np.array_equal(r[3], V), case[0]
    assert n_multi >= 1


@pytest.mark.parametrize("windowed", [False, True], ids=["whole", "windowed"])
@pytest.mark.parametrize("cfg", sorted(REPLAY_CFGS))
def test_every_rebuilt_term_is_the_twins_after_the_forward_run(cfg, windowed):
    """AUGX_EXACT_MULTICLASS=0: the Viterbi run scores an interior with the class of its end base and nothing is replayed after it; the
    replay after the forward run, from which cells of the forward matrix are alive, does the patching.  The cells alive in the forward
    matrix are those alive in the Viterbi matrix: the same requests, the same terms.  (The cells of this Viterbi run are the twin's
    with its caches off.)"""
    res, (cnt, terms, hist) = emu_run(cfg, windowed, env=(("AUGX_EXACT_MULTICLASS", "0"),), forward=True)
    m = model(cfg)
    for i, case in enumerate(cases(cfg)):
        name, seq, ik, tk = case
        (rc, lnv, path, V, gc), want, sites, flushes = twin_of(cfg, case)
        assert_terms_equal(terms.get(i, {}), want, (cfg, name))
        if cfg in REPLAY_DENSE:
            assert hist.get(i, []) == site_changes(sites), name
        plain = twin_decode(m.tables_ptr, seq, m.n_states, cells=True, init_kind=ik, term_kind=tk, cache=False)
        assert res[i][1] == plain[1] and np.array_equal(res[i][3], plain[3]), name
        assert np.array_equal(np.isfinite(res[i][5]), np.isfinite(V)), name


@pytest.mark.parametrize("slow", [False, True], ids=["skipping", "call_by_call"])
@pytest.mark.parametrize("windowed", [False, True], ids=["whole", "windowed"])
@pytest.mark.parametrize("cfg", REPLAY_DENSE)
def test_every_site_value_is_computed_by_the_twins_asker_with_its_class(cfg, windowed, slow):
    """the history of the acceptor sites: which column and state computes a site's value, with which class, in the order of the calls;
    how often the memo is emptied; the walk that skips what it knows to be in the memo against the plain call-by-call one"""
    res, (cnt, terms, hist) = emu_run(cfg, windowed, env=(("AUGX_MEMO_SLOW", "1"),) if slow else ())
    total = 0
    for i, case in enumerate(cases(cfg)):
        (rc, lnv, path, V, gc), want, sites, flushes = twin_of(cfg, case)
        assert hist.get(i, []) == site_changes(sites), case[0]
        total += flushes
        assert np.array_equal(res[i][3], V), case[0]
    assert cnt["flushes"] == total
    assert (cnt["skips"] == 0) == slow


@pytest.mark.parametrize("cfg", sorted(REPLAY_CFGS))
def test_windowed_mode_is_whole_mode(cfg):
    """the route of the device library against the emulator's own: patches, site history, cells, score, path and every counter"""
    whole, (cw, tw, hw) = emu_run(cfg, False)
    wind, (cd, td, hd) = emu_run(cfg, True)
    assert tw == td and hw == hd and cw == cd
    for a, b in zip(whole, wind):
        assert a[:3] == b[:3] and np.array_equal(a[3], b[3])


# counters no input can reach, with the reason
UNREACHABLE = {
    "add_same": "get() adds a length only after it found no entry of that length in the list (the reference's warning 'tried to add "
                "snippet of same length' never fires either)",
    "map_fallback": "a request of the window t0..t1 and its recursive requests end at bases j - d .. j with t0 <= j <= t1: inside the flat "
                    "range that window() lays out from t0 - d - 64",
    "below_row0": "the predecessor end of a request lies at most d before its end base j >= t0, the rows begin d + 2 before t0",
    "extras": "a site whose longass state would end past the piece is asked for by utr5term alone, from the last W + Ae + 63 columns at most; "
              "no class step lies within GCwinsize / 2 >= 300 bases of the end, so the asker's class is that of the last base",
}


def test_the_inputs_reach_every_path_of_the_replays():
    """the counters of the replays over all inputs, Viterbi and forward runs, whole mode (the windowed mode counts the same: above):
    every path is taken, but the ones that cannot be -- asserted 0, with the reason.  The steps of the edge inputs lie where the
    docstring of helpers.replay_edge_cases says."""
    tot = {}
    for cfg in sorted(REPLAY_CFGS):
        tot = merge_counters(tot, emu_run(cfg, False)[1][0])
        tot = merge_counters(tot, emu_run(cfg, False, env=(("AUGX_EXACT_MULTICLASS", "0"),), forward=True)[1][0])
    # a decomposition of mixed classes that gives the term the candidate has: the forward run's replay of what the Viterbi run patched
    exact_fwd = emu_run("human_w600", False, forward=True)[1][0]
    assert exact_fwd["mixed_same"] > 0 and exact_fwd["patch_fwd"] + exact_fwd["patch_rev"] == sum(len(twin_of("human_w600", c)[1]) for c in cases("human_w600"))
    tot = merge_counters(tot, exact_fwd)
    late = ("late_calls", "late_flushes", "vit_diffs")  # (calls after the sweep: test_late_calls_* below)
    for k in SNIP_COUNTERS + ASS_COUNTERS + ("tss_changed",):
        if k in UNREACHABLE:
            assert tot[k] == 0, (k, tot[k], UNREACHABLE[k])
        elif k not in late:
            assert tot[k] > 0, k
    assert tot["max_blocks"] > 256 and model("nasonia_w1000").n_states == 47 and emu_block_size(model("nasonia_w1000").tables_ptr) == 8
    # the class steps of the inputs made for the piece ends
    for cfg in ("human_w600", "human_utr_w600"):
        d = emu_model_dims(model(cfg).tables_ptr)["d"]
        got = {}
        for case in cases(cfg)[:4]:
            gc = twin_of(cfg, case)[0][4].tolist()
            got[case[0]] = (len(gc), [j for j in range(1, len(gc)) if gc[j] != gc[j - 1]])
        n, st = got["step_start"]
        assert len(st) == 1 and st[0] - d - 64 < 0 and st[0] + 2 * d + 64 <= n - 1
        n, st = got["step_end"]
        assert len(st) == 1 and st[0] - d - 64 >= 1 and st[0] + 2 * d + 64 > n - 1
        n, st = got["step_both"]
        assert len(st) == 2 and st[0] - d - 64 < 0 and st[1] + 2 * d + 64 > n - 1
    one = emu_run("human_w600", False)[1][0]
    assert one["clamp_start"] == 3 and one["clamp_end"] == 3 and one["merged"] == 2 and one["col0_req"] > 0


def test_late_calls_go_on_from_the_memo_the_sweep_left():
    """the aSSProb memo lives on through the sampled paths (sampler.h: memoStep): a gene between AG-rich flanks, 20 sampled paths --
    the memo is emptied by a call after the sweep; a second piece on which the back-tracking of the Viterbi path values sites under
    another class than the sweep did"""
    from helpers import _ag_rich
    gene = dict(golden_inputs())["HS04636"].upper()
    seq = _ag_rich(3000, 0.70, 1, 5) + gene[4000:9000] + _ag_rich(3000, 0.34, 2, 5)
    m = model("human_utr_w600", sample="100")
    emu_decode(m.tables_ptr, [seq], m.n_states, samples=20)
    cnt = emu_replay_log()[0]
    assert cnt["late_calls"] > 1000 and cnt["late_flushes"] >= 1 and cnt["flushes"] >= 1
    # The back-tracking of the Viterbi path asks again for the sites of its UTR exon steps: a site that the sweep has emptied out of the
    # memo since, or computed again under another class, gets another class than the step saw during the sweep (sampler.h:
    # SamplePiece::memoVitDiffs counts those candidates; the piece above has none, this one was found by a search over flanks and
    # cuts of the gene driven by the counter)
    seq = _ag_rich(3500, 0.70, 687, 4) + gene[5000:8000] + _ag_rich(2500, 0.34, 686, 3)
    emu_decode(m.tables_ptr, [seq], m.n_states, samples=1)
    cnt2 = emu_replay_log()[0]
    assert cnt2["vit_diffs"] > 0 and cnt2["flushes"] >= 1 and cnt2["late_calls"] > 0


@needs_ref
@pytest.mark.parametrize("cfg", sorted(REPLAY_CFGS))
def test_forward_matrix_of_the_edge_inputs_is_the_live_references(cfg, tmp_path):
    """every forward variable of the edge inputs against the live reference, to the project's 1e-9 |ref| + 5e-9 (pieces decoded as
    whole sequences: the reference run knows no interior cuts)"""
    species, opts = REPLAY_CFGS[cfg]
    cs = [c for c in replay_edge_cases()[cfg] if c[2] == 0 and c[3] == 0]
    fa = str(tmp_path / "e.fa")
    write_fasta(fa, [(c[0], c[1]) for c in cs])
    ref = ref_forward(fa, species, ["--%s=%s" % kv for kv in opts.items() if kv[0] != "sample"])
    assert len(ref) == len(cs)
    m = model(cfg, sample="100")
    res = emu_decode(m.tables_ptr, [c[1] for c in cs], m.n_states, forward=True)
    for c, r, w in zip(cs, res, ref):
        F, want = r[5], w
        assert np.array_equal(np.isfinite(F), np.isfinite(want)), c[0]
        both = np.isfinite(want)
        assert np.all(np.abs(F[both] - want[both]) <= 1e-9 * np.abs(want[both]) + 5e-9), c[0]


ALL_SPECIES = sorted(set(v[0] for v in {**GOLDEN_CFGS, **MORE_CFGS}.values()) | {"caenorhabditis", "maize", "Vitrella_brassicaformis", "chlamy2011", "tetrahymena"})


# the species fixtures that load with --UTR=on; the others have no UTR parameters (no *_utr_probs.pbl, no /UtrModel/ keys) or an intron
# Markov order the UTR states do not support, and Model() says so in these words
UTR_SPECIES = {"human", "fly", "caenorhabditis", "chlamy2011"}
NO_UTR_MODEL = ("_utr_probs.pbl", 'no such key "/UtrModel/', "UTR states with an intron Markov order other than the exon order")


def test_the_utr_species_are_among_the_fixtures():
    assert UTR_SPECIES <= set(ALL_SPECIES)


@pytest.mark.parametrize("species", ALL_SPECIES)
def test_sites_past_the_end_fit_the_slots_the_memo_replay_keeps(species):
    """kMemoSites keeps 8 slots per piece for acceptor sites whose longass state would end past the piece; there are up to ass_end of
    them.  A UTR model with more is refused where a decoder is created (layout.h: chooseDenseBlock); every UTR fixture model passes:
    the species of UTR_SPECIES must load and reach the check, any other may only fail with the refusal of --UTR=on."""
    try:
        m = ax.Model(config_path(), species, UTR="on", softmasking="0")
    except ax.AugxError as e:
        # only the refusal of --UTR=on for a species without (usable) UTR parameters leaves nothing to check
        assert species not in UTR_SPECIES, (species, e)
        assert any(w in str(e) for w in NO_UTR_MODEL), (species, e)
        return
    assert species in UTR_SPECIES, species
    out = (ctypes.c_int * 3)()
    ctypes.CDLL(EMU_LIB).emu_ass_past_end(m.tables_ptr, out)
    assert out[2] == 1 and out[1] == 8 and 0 <= out[0] <= out[1]
    assert emu_block_size(m.tables_ptr) in (8, 4, 2)  # (the check passed)


def test_a_model_with_more_sites_past_the_end_is_refused():
    m = ax.Model(config_path(), "human", UTR="on", softmasking="0")
    t = ctypes.cast(m.tables_ptr, ctypes.c_void_p)
    out = (ctypes.c_int * 3)()
    E = ctypes.CDLL(EMU_LIB)
    E.emu_ass_past_end(m.tables_ptr, out)
    E.emu_dense_block_with_ass_end.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert E.emu_dense_block_with_ass_end(t, out[0]) in (4, 2)
    assert E.emu_dense_block_with_ass_end(t, 8) in (4, 2, -1)   # (8 fits the slots; another check may still refuse the model)
    assert E.emu_dense_block_with_ass_end(t, 9) == -2            # refused, by this check
