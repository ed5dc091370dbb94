"""Segments for the dense kernels on the GPU (kDenseSeg<BLK, TIES>, dense.h: denseTiles; kSegFinalize; kDenseBacktrace over regions of
different offsets): the records of tests/test_dense_seg_cpu.py through Decoder / Batch against the oracle twin, which knows no
segments -- augx_batch_cells, score, path and near ties bit for bit, the plan read back with where every fix-up stopped; the default
plan; the executable with its defaults on one 1 Mbp record against the reference binary's GFF; the second run after the cache replays;
the refusal of the models with two intergenic states."""
import os
import subprocess
import tarfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from dense_seg_cases import *

EXE = os.path.join(ROOT, "augustus_amd", "bin", "augustus")


def _decode(m, seqs, ties=True):
    d = ax.Decoder(m, 0)
    d.count_near_ties(ties)
    b = ax.Batch(d, seqs)
    b.decode()
    return d, b


def _check(m, cfg, b, seqs, ties=True):
    res = b.paths()
    near = b.near_ties() if ties else None
    for i, (seq, r) in enumerate(zip(seqs, res)):
        T = twin_want(m, cfg, seq)
        assert r.status == T.rc == 0, (i, r.status, T.rc)
        assert np.array_equal(b.cells(i), T.V), i
        assert r.ln_viterbi == T.lnv and r.states == T.path, i
        if ties:
            assert near[i] == T.counts(TIES_PRODUCT_EPS)[0], i


@pytest.mark.parametrize("cfg,blk", SEG_MODELS)
def test_three_segments(monkeypatch, cfg, blk):
    """the three-segment record with the model's own check length (the fix-ups write seg_stop; at least one converges), then with an
    unreachable one (every fix-up gives up at its tlim, the continuation of the first runs to the end); decoded twice each"""
    m = seg_model(cfg, blk, monkeypatch)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    seq = plain_record(m)
    last = (len(seq) + 63) // 64 - 1
    for give_up in (False, True):
        if give_up:
            monkeypatch.setenv("AUGX_SEG_CHECK_TILES", "100000")
        d, b = _decode(m, [seq])
        for turn in range(2):
            if turn:
                b.decode()
            _check(m, cfg, b, [seq])
            plan = b.plan()
            assert len(plan["segs"]) == 3 and plan["n_runs"] == 0 and plan["check_tiles"] == check_tiles(m)
            if give_up:
                assert gave_up(plan) == [1, 2] and int(plan["seg_stop2"][1]) == last, plan
                assert [int(-2 - plan["seg_stop"][q]) for q in (1, 2)] == [int(plan["segs"][q][4]) for q in (1, 2)]
            else:
                assert converged(plan), plan
                assert all(int(plan["seg_stop"][q]) <= int(plan["segs"][q][4]) for q in converged(plan))
        b.close()
        d.close()


@pytest.mark.parametrize("cfg,blk", [("human_utr", "4"), ("maize", "8")])
def test_run_of_n_and_gene_across_a_cut(monkeypatch, cfg, blk):
    """one batch: the record whose run of N spans a cut (a fix-up gives up) and the one with a gene across the cut, without the
    near-tie build (kDenseSeg<BLK, false>)"""
    m = seg_model(cfg, blk, monkeypatch)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    seqs = [nrun_record(m), gene_record(m)]
    d, b = _decode(m, seqs, ties=False)
    _check(m, cfg, b, seqs, ties=False)
    plan = b.plan()
    assert [int((plan["segs"][:, 0] == p).sum()) for p in range(2)] == [3, 2]
    assert gave_up(plan) and gave_up(plan)[0] < 3, plan
    b.close()
    d.close()


def test_default_plan(monkeypatch):
    """no environment variable: a record long enough is cut (fewer pieces than workgroup slots), 300 short ones are not"""
    monkeypatch.delenv("AUGX_SEG_LEN", raising=False)
    m = seg_model("human_utr", "4", monkeypatch)
    seq = gene_record(m)
    d, b = _decode(m, [seq])
    assert len(b.plan()["segs"]) == 2
    _check(m, "human_utr", b, [seq])
    b.close()
    short = [random_dna(400 + 7 * i, 1000 + i) for i in range(300)]
    b = ax.Batch(d, short)
    b.decode()
    plan = b.plan()
    assert len(plan["segs"]) == 300 and (plan["seg_stop"] == -1).all()
    for i in (0, 150, 299):
        T = twin_want(m, "human_utr", short[i])
        r = b.paths()[i]
        assert r.status == T.rc == 0 and r.ln_viterbi == T.lnv and r.states == T.path and np.array_equal(b.cells(i), T.V)
    b.close()
    d.close()


@pytest.fixture(scope="module")
def genome_fa(tmp_path_factory):
    d = tmp_path_factory.mktemp("big_seg")
    with tarfile.open(os.path.join(GOLDEN, "big_inputs.tar.gz")) as t:
        t.extractall(str(d))
    return str(d / "genome.fa")


@pytest.mark.parametrize("gold,extra", [("golden_big_human_utr.gff", ["--UTR=on"]), ("golden_big_human_utr_sampled.gff", ["--UTR=on", "--sample=100"])])
def test_cli_defaults_cut_the_one_mbp_record(genome_fa, gold, extra):
    """the executable with its defaults on the single 1 Mbp human record: the Viterbi decode is cut (the plan line of AUGX_TIMING), the
    forward pass is not, the memo replay reads the segmented matrix; GFF byte-identical to the reference binary's"""
    env = dict(os.environ, AUGUSTUS_CONFIG_PATH=config_path(), AUGX_TIMING="1")
    env.pop("AUGX_SEG_LEN", None)
    env.pop("AUGX_SEG_CHECK_TILES", None)
    env.pop("AUGX_BLK", None)
    r = subprocess.run([EXE, "--species=human"] + extra + [genome_fa], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert gff_body(r.stdout) == open(os.path.join(GOLDEN, gold)).read().splitlines()
    lines = [l for l in r.stderr.splitlines() if "trellis plan:" in l]
    assert lines, r.stderr[-2000:]
    nseg = int(lines[0].split("trellis plan:")[1].split()[0])
    assert nseg > 1 and " of 1 pieces" in lines[0], lines[0]


def test_exact_mode_second_run_is_cut(monkeypatch):
    """a UTR record with several GC classes in exact mode (the default): the reference's caches are replayed from the aliveness of the
    segmented matrix, and the second run takes the same passes.  The twin without the restated caches differs, so the replays count"""
    monkeypatch.delenv("AUGX_EXACT_MULTICLASS", raising=False)
    m = seg_model("human_utr", "4", monkeypatch)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(m)))
    (_, seq), = gc_step_records(1, 31, parts=40, lo=4000, hi=6000)
    assert len(seq) >= 2 * seg_len(m)
    T = twin_want(m, "human_utr", seq)
    rc0, lnv0, path0, V0, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=True, cache=False)
    assert rc0 == 0 and not np.array_equal(V0, T.V)
    d, b = _decode(m, [seq])
    assert len(b.plan()["segs"]) >= 2
    _check(m, "human_utr", b, [seq])
    b.close()
    d.close()


def test_two_intergenic_states_uncut(monkeypatch):
    m = seg_model("human_exactlyone", "8", monkeypatch)
    monkeypatch.setenv("AUGX_SEG_LEN", str(seg_len(seg_model("human_utr"))))
    seq = gene_record(seg_model("human_utr"))
    rc, lnv, path, V, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
    d, b = _decode(m, [seq], ties=False)
    plan = b.plan()
    assert len(plan["segs"]) == 1 and (plan["seg_stop"] == -1).all()
    r, = b.paths()
    assert r.status == rc and np.array_equal(b.cells(0), V)
    if rc == 0:
        assert r.ln_viterbi == lnv and r.states == path
    b.close()
    d.close()
