"""The replays of the reference's call-history caches on the device, value by value (tests/test_emu_replay.py has the why and the same
checks on the emulator, and shows from the replays' counters which paths the inputs take).  On the device the replay runs in windowed
mode: kGatherWindows packs what the windows of a piece read, host workers replay one piece after the other on a stream of their own,
kPatchItems writes the rebuilt terms back; kTssReplay, kMemoSites, kMemoGates and kAssPatch do the same for the two caches of the UTR
states.  Through the read-only hooks of a decoder created with AUGX_DEBUG_CELLS=1 (Batch.replay_hooks):
- every rebuilt candidate term is the one of the oracle twin's cache log, by (end base, state, predecessor end), bit for bit, and nothing
  else is rebuilt; every change of an acceptor site's value has the twin's asker and class; the counters are the emulator's;
- cells, score and path are the twin's; a second decode rebuilds the same terms and leaves the same cells;
- after Batch.decode() and after Batch.forward() with the Viterbi run's replay off, both piece orders, 47 and 71 states;
- 13 two-class pieces among single-class ones in one batch: more than the replay has workers when it reads a matrix, piece indices
  above 0 in the offsets of the site slots; the same with two workers (AUGX_REPLAY_THREADS is read once: a fresh child process);
- with the replays switched off the cells differ."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *


@pytest.fixture(autouse=True)
def _debug_hooks(monkeypatch):
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    for k in ("AUGX_EXACT_MULTICLASS", "AUGX_NO_MEMO", "AUGX_NO_ASSMEMO", "AUGX_EMU_WINDOWED", "AUGX_MEMO_SLOW"):
        monkeypatch.delenv(k, raising=False)


def _batch(d, cs):
    return ax.Batch(d, [c[1] for c in cs], init_kind=[c[2] for c in cs], term_kind=[c[3] for c in cs])


def _check_values(cfg, b, cs, cells=True, patched=True):
    """patches, site history, score, path and cells of a decoded batch against the twin; returns the counters"""
    cnt, terms, hist = batch_replay_log(b)
    res = b.paths()
    flushes = 0
    for i, case in enumerate(cs):
        (rc, lnv, path, V, gc), want, sites, fl = replay_twin(cfg, case)
        if patched:
            assert_terms_equal(terms.get(i, {}), want, (cfg, case[0], i))
        if cfg in REPLAY_DENSE:
            assert hist.get(i, []) == site_changes(sites), (case[0], i)
            flushes += fl
        assert res[i].status == rc == 0 and res[i].ln_viterbi == lnv and res[i].states == path, (case[0], i)
        if cells:
            assert np.array_equal(b.cells(i), V), (case[0], i)
    if cfg in REPLAY_DENSE:
        assert cnt["flushes"] == flushes
    return cnt, terms


def _emu_counters(cfg, cs, forward=False):
    """the counters of the emulator's replay of the same batch, in the windowed mode the device runs"""
    m = replay_model(cfg)
    os.environ["AUGX_EMU_WINDOWED"] = "1"
    try:
        emu_decode(m.tables_ptr, [c[1] for c in cs], m.n_states, init_kind=[c[2] for c in cs], term_kind=[c[3] for c in cs], forward=forward)
        return emu_replay_log()[0]
    finally:
        del os.environ["AUGX_EMU_WINDOWED"]


@pytest.mark.parametrize("order", ["given", "reversed"])
@pytest.mark.parametrize("cfg", sorted(REPLAY_CFGS))
def test_gpu_decode_rebuilds_the_twins_values(cfg, order):
    cs = replay_edge_cases()[cfg]
    cs = cs if order == "given" else cs[::-1]
    d = ax.Decoder(replay_model(cfg), 0)
    b = _batch(d, cs)
    b.decode()
    cnt, terms = _check_values(cfg, b, cs)
    assert cnt == _emu_counters(cfg, cs)
    assert sum(len(t) for t in terms.values()) > 0
    first = [b.cells(i) for i in range(len(cs))]
    b.decode()  # (the same batch again: the candidates are made afresh, the same terms are rebuilt, nothing else)
    cnt2, terms2 = _check_values(cfg, b, cs)
    assert terms2 == terms and cnt2 == cnt
    assert all(np.array_equal(b.cells(i), first[i]) for i in range(len(cs)))
    # the forward run after it replays once more: every mixed request gives the term the candidate has by now
    b.forward()
    cntF, termsF, histF = batch_replay_log(b)
    assert not termsF and cntF["mixed_same"] == cnt["patch_fwd"] + cnt["patch_rev"] + cnt["mixed_same"] and cntF["patch_fwd"] == cntF["patch_rev"] == 0
    for i, case in enumerate(cs):
        assert np.array_equal(np.isfinite(b.forward_cells(i)[0]), np.isfinite(first[i])), case[0]
    b.close()
    d.close()


@pytest.mark.parametrize("cfg", sorted(REPLAY_CFGS))
def test_gpu_forward_rebuilds_the_twins_values(monkeypatch, cfg):
    """AUGX_EXACT_MULTICLASS=0: nothing is replayed after the Viterbi run (its cells are the twin's with the caches off); the replay
    after the forward run reads which cells of the forward matrix are alive"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")
    cs = replay_edge_cases()[cfg]
    m = replay_model(cfg)
    d = ax.Decoder(m, 0)
    b = _batch(d, cs)
    b.decode()
    cnt0, terms0, hist0 = batch_replay_log(b)
    assert not terms0 and not hist0
    for i, (name, seq, ik, tk) in enumerate(cs):
        plain = twin_decode(m.tables_ptr, seq, m.n_states, cells=True, init_kind=ik, term_kind=tk, cache=False)
        assert np.array_equal(b.cells(i), plain[3]), name
    b.forward()
    cnt, terms, hist = batch_replay_log(b)
    for i, case in enumerate(cs):
        (rc, lnv, path, V, gc), want, sites, fl = replay_twin(cfg, case)
        assert_terms_equal(terms.get(i, {}), want, (cfg, case[0]))
        if cfg in REPLAY_DENSE:
            assert hist.get(i, []) == site_changes(sites), case[0]
        assert np.array_equal(np.isfinite(b.forward_cells(i)[0]), np.isfinite(V)), case[0]
    assert cnt == _emu_counters(cfg, cs, forward=True)
    b.close()
    d.close()


def check_batch_of_13(cfg):
    cs = [(n, s, 0, 0) for n, s in replay_batch_pieces(13, distinct=4 if cfg in REPLAY_DENSE else None)]
    d = ax.Decoder(replay_model(cfg), 0)
    for order in (cs, cs[::-1]):
        b = _batch(d, order)
        b.decode()
        cnt, terms = _check_values(cfg, b, order)
        assert sorted(terms) == [i for i, c in enumerate(order) if c[0].startswith("two")] and len(terms) == 13
        assert cnt["windows"] == 26
        b.close()
    d.close()


@pytest.mark.parametrize("cfg", ["human", "human_utr"])
def test_gpu_more_multiclass_pieces_than_replay_workers(cfg):
    check_batch_of_13(cfg)


def test_gpu_two_replay_workers():
    """AUGX_REPLAY_THREADS=2, read when a process first replays: a worker takes one piece after the other on its stream"""
    env = dict(os.environ, AUGX_REPLAY_THREADS="2", AUGX_DEBUG_CELLS="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    code = "import test_gpu_replay as t; t.check_batch_of_13('human'); t.check_batch_of_13('human_utr'); print('two workers ok')"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=os.path.join(ROOT, "tests"), timeout=300)
    assert r.returncode == 0 and "two workers ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("cfg,switch", [("human_w600", "AUGX_EXACT_MULTICLASS"), ("human_utr_w600", "AUGX_NO_ASSMEMO")])
def test_gpu_the_replays_are_what_changes_the_cells(monkeypatch, cfg, switch):
    """without the replay of the snippet cache (47 states) / of the aSSProb memo and the TSS windows (71 states) cells differ from the
    twin's; AUGX_NO_MEMO does the same to the forward matrix"""
    cs = replay_edge_cases()[cfg]
    m = replay_model(cfg)

    def run(fwd):
        d = ax.Decoder(m, 0)
        b = _batch(d, cs)
        b.decode()
        out = [b.cells(i) for i in range(len(cs))]
        if fwd:
            b.forward()
            out = [b.forward_cells(i)[0] for i in range(len(cs))]
        log = batch_replay_log(b)
        b.close()
        d.close()
        return out, log
    on, log_on = run(False)
    monkeypatch.setenv(switch, "0" if switch == "AUGX_EXACT_MULTICLASS" else "1")
    off, log_off = run(False)
    assert sum(int(not np.array_equal(a, c)) for a, c in zip(on, off)) >= 2
    if switch == "AUGX_NO_ASSMEMO":
        assert log_on[2] and not log_off[2] and log_off[1] == log_on[1]  # (the site history is gone, the snippet terms are not)
    else:
        assert log_on[1] and not log_off[1]
    monkeypatch.delenv(switch)
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")
    f_on, _ = run(True)
    monkeypatch.setenv("AUGX_NO_MEMO", "1")
    f_off, log = run(True)
    assert not log[1] and not log[2]
    assert sum(int(not np.array_equal(a, c)) for a, c in zip(f_on, f_off)) >= 2
