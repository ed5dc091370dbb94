"""The inputs made for the far-window and overflow paths of the trellis and forward kernels (helpers.trellis_edge_cases,
helpers.trellis_edge_long; tests/test_emu_trellis.py shows from the emulator's counters that they take those paths) on the GPU:
- kTrellis at block sizes 8, 4 and 2, role-specialised and as the common body that flags near ties, every batch decoded twice and in
  both orders, whole and cut into segments (fix-ups that converge; an unreachable check length: continuations and the last pass):
  every cell, the score and the path equal the oracle twin's bit for bit -- where the value a candidate reads back from HBM was
  stored by another wavefront a tile earlier, which the sequential emulator cannot get wrong;
- the same with the trellis kernels built for the smallest LDS windows kernels.h admits (augustus_amd/libaugx_smallwin.so, loaded by
  a fresh child process through AUGX_LIB), where those reads are the common case;
- kForward against every forward variable of the live reference, cold and heated, and bit-equal run after run where thousands of
  LDS atomics hit one cell."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *

SEG_ENVS = [{"AUGX_SEG_LEN": "77000"}, {"AUGX_SEG_LEN": "77000", "AUGX_SEG_CHECK_TILES": "100000"}]
_want = {}


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """exact mode off, as in test_gpu_parity.py: decoders are created with the first pass on its own, and the twin's restatement of the
    snippet cache is off with it"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")


def _twin(m, seq, tag):
    """the twin's (score, path, cells) of one record under model m; tag names the model's species and options (the twin does not know
    AUGX_BLK, the segments or the near-tie build: one decode serves them all)"""
    key = (tag, seq)
    if key not in _want:
        rc, lnv, path, V, _ = twin_decode(m.tables_ptr, seq, m.n_states, cells=True)
        assert rc == 0
        _want[key] = (lnv, path, V)
    return _want[key]


def _check_batch(m, b, seqs, tag):
    res = b.paths()
    assert len(res) == len(seqs)
    for i, (seq, r) in enumerate(zip(seqs, res)):
        lnv, path, V = _twin(m, seq, tag)
        assert r.status == 0, i
        assert r.ln_viterbi == lnv and r.states == path, i
        assert np.array_equal(b.cells(i), V), i


def _decode_and_check(m, seqs, ties, tag="human"):
    d = ax.Decoder(m, 0)
    d.count_near_ties(ties)  # (True: batches created from now on run kTrellis<., ., true>, the common body)
    for order in (seqs, seqs[::-1]):
        b = ax.Batch(d, order)
        b.decode()
        _check_batch(m, b, order, tag)
        b.decode()  # (the same batch again: the buffers hold what the first decode left)
        _check_batch(m, b, order, tag)
        b.close()
    d.close()


def check_library(blks, ties, segments):
    """the body of the tests below, for the library this process has loaded (the caller sets AUGX_EXACT_MULTICLASS=0)"""
    os.environ["AUGX_DEBUG_CELLS"] = "1"
    seqs = [s for _, s in trellis_edge_cases()]
    for blk in blks:
        os.environ["AUGX_BLK"] = blk
        m = ax.Model(config_path(), "human")
        for t in ties:
            _decode_and_check(m, seqs, t)
    os.environ["AUGX_BLK"] = "8"
    for env in SEG_ENVS if segments else ():
        saved = {k: os.environ.get(k) for k in ("AUGX_SEG_LEN", "AUGX_SEG_CHECK_TILES")}
        os.environ.update(env)
        try:
            m = ax.Model(config_path(), "human")
            for t in ties:
                _decode_and_check(m, [trellis_edge_long()] + seqs[2:5], t)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
    os.environ.pop("AUGX_BLK", None)
    os.environ.pop("AUGX_DEBUG_CELLS", None)


@pytest.mark.parametrize("ties", [False, True], ids=["roles", "common_body"])
@pytest.mark.parametrize("blk", ["8", "4", "2"])
def test_gpu_trellis_edge_cases_bit_identical_to_oracle(monkeypatch, blk, ties):
    monkeypatch.setenv("AUGX_BLK", blk)  # (restored after the test; check_library sets it itself)
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    check_library([blk], [ties], False)


@pytest.mark.parametrize("species", ["fly", "caenorhabditis"])
def test_gpu_trellis_edge_cases_other_models(monkeypatch, species):
    """a second species at block size 8 and the model that takes block size 4 by itself"""
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    m = ax.Model(config_path(), species, UTR="off", sample="0", softmasking="0")
    _decode_and_check(m, [s for _, s in trellis_edge_cases()], False, species)


@pytest.mark.parametrize("ties", [False, True], ids=["roles", "common_body"])
@pytest.mark.parametrize("env", SEG_ENVS, ids=["check", "nocheck"])
def test_gpu_trellis_edge_long_segments(monkeypatch, env, ties):
    """five segments with far predecessors across the seams and a fix-up that starts inside a run of N (helpers.trellis_edge_long);
    with an unreachable check length every fix-up gives up: three continuations, the rest by the last pass"""
    monkeypatch.setenv("AUGX_DEBUG_CELLS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = ax.Model(config_path(), "human")
    seqs = [s for _, s in trellis_edge_cases()]
    _decode_and_check(m, [trellis_edge_long()] + seqs[2:5], ties)


def test_gpu_trellis_small_windows():
    """the trellis kernels built with AUGX_ITEM_CAP=1024 AUGX_LIST_WIN=128 AUGX_VIG_WIN=128 (Makefile: libaugx_smallwin.so): the same bit
    equality at the three block sizes, whole and in segments.  A fresh process: the library is chosen when augustus_amd is imported"""
    assert os.path.exists(SMALLWIN_LIB), "augustus_amd/libaugx_smallwin.so is missing: `make product` builds it"
    env = dict(os.environ, AUGX_LIB=SMALLWIN_LIB, AUGX_EXACT_MULTICLASS="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    for k in ("AUGX_BLK", "AUGX_SEG_LEN", "AUGX_SEG_CHECK_TILES"):
        env.pop(k, None)
    code = ("import augustus_amd as ax, test_gpu_trellis as t; assert ax.LIB_PATH.endswith('libaugx_smallwin.so'); "
            "t.check_library(['8', '4', '2'], [False], True); t.check_library(['8'], [True], False); print('small windows ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=os.path.join(ROOT, "tests"), timeout=900)
    assert r.returncode == 0 and "small windows ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@needs_ref
@pytest.mark.parametrize("cfg,t", [("human_nosm", 0), ("fly", 0), ("human_nosm", 3), ("fly", 3)])
def test_gpu_forward_edge_cases_match_reference(tmp_path, monkeypatch, cfg, t):
    """every forward variable of the records of trellis_edge_cases on the device against the live reference: identical live cells,
    |ln F - reference| <= 1e-9 |reference| + 5e-9, cold and at --temperature=3; and a second forward run of the
    same batch gives the same bits -- the fixed-point sum of a cell does not depend on the order its 3990 atomics arrive in"""
    monkeypatch.delenv("AUGX_EXACT_MULTICLASS")  # (the replay of the reference's snippet cache: two records have two classes under human)
    species, opts = GOLDEN_CFGS[cfg]
    recs = trellis_edge_cases()
    fa = str(tmp_path / "f.fa")
    write_fasta(fa, recs)
    extra = ["--%s=%s" % kv for kv in opts.items() if kv[0] != "sample"] + (["--temperature=%d" % t] if t else [])
    Fref = ref_forward(fa, species, extra)
    m = ax.Model(config_path(), species, **{**opts, "sample": "100", "temperature": str(t)})
    d = ax.Decoder(m, 0)
    b = ax.Batch(d, [s for _, s in recs])
    b.decode()
    b.forward()
    first = [b.forward_cells(i) for i in range(len(recs))]
    b.forward()
    worst = 0.0
    for i, ((name, seq), fr, r) in enumerate(zip(recs, Fref, b.paths())):
        F, lnp = b.forward_cells(i)
        assert np.array_equal(F.view(np.uint64), first[i][0].view(np.uint64)) and lnp == first[i][1], name
        assert np.array_equal(np.isfinite(F), np.isfinite(fr)), name
        both = np.isfinite(F)
        diff = np.abs(F[both] - fr[both])
        worst = max(worst, float(np.max(diff / (np.abs(fr[both]) + 5))))
        assert np.all(diff <= 1e-9 * np.abs(fr[both]) + 5e-9), name
        assert lnp >= r.ln_viterbi
    print("device forward %s t=%d: largest |ln F - reference| / (|reference| + 5) = %.3g" % (cfg, t, worst))
    b.close()
    d.close()
