"""Records, models and yardsticks of the segment tests of the dense kernels (tests/test_dense_seg_cpu.py, tests/test_gpu_dense_seg.py).

Sizes follow from the model: `check_tiles` is read from augx_plan_segments, AUGX_SEG_LEN = 5 * check_tiles * 64 is the shortest segment
the planner makes, and the shortest record it cuts into three segments has 15 * check_tiles tiles.  The yardstick is the oracle twin
(helpers.twin_decode), which knows no segments; it is computed once per (configuration, record)."""
import ctypes
import os
import random

import numpy as np

import augustus_amd as ax
from helpers import *

SEG_EMU_LIB = os.path.join(ROOT, "build", "libaugx_emu_dense_seg.so")
# (configuration, block size): the 71-state model with UTR states at both block sizes it runs at, and a 47-state model of the dense family
SEG_CFGS = {
    "human_utr": ("human", {"UTR": "on"}),
    "maize": ("maize", {"UTR": "off", "sample": "0", "softmasking": "0"}),
    "human_exactlyone": ("human", {"genemodel": "exactlyone"}),   # two intergenic states: never cut
    "human": ("human", {}),                                       # the trellis family
}
SEG_MODELS = [("human_utr", "4"), ("human_utr", "2"), ("maize", "8")]
_models, _want = {}, {}


def seg_model(cfg, blk=None, monkeypatch=None):
    """the model of a configuration; blk: AUGX_BLK for the test (it is read when a decoder is created or an emulator run starts)"""
    if blk is not None:
        monkeypatch.setenv("AUGX_BLK", blk)
    if cfg not in _models:
        species, opts = SEG_CFGS[cfg]
        _models[cfg] = ax.Model(config_path(), species, **opts)
    return _models[cfg]


def check_tiles(m):
    return ax.plan_segments(m, [1000], 256)["check_tiles"]


def seg_len(m):
    """AUGX_SEG_LEN of the tests, in bases: the shortest segment"""
    return 5 * check_tiles(m) * 64


def three_seg_bases(m):
    """length of the shortest record AUGX_SEG_LEN = seg_len(m) cuts into three segments (the last tile holds one base)"""
    return (15 * check_tiles(m) - 1) * 64 + 1


def plain_record(m, seed=99):
    return random_dna(three_seg_bases(m), seed)


def nrun_record(m, seed=98):
    """the same with a run of N from before the first cut to beyond the last tile the fix-up of the second segment may rewrite: inside the
    run every state decays alike, a dead start and the true run keep their difference, and the fix-up gives up"""
    ck = check_tiles(m)
    s = random_dna(three_seg_bases(m), seed)
    a, b = (5 * ck - 40) * 64, (10 * ck - ck + 8) * 64
    return s[:a] + "N" * (b - a) + s[b:]


def gene_record(m, seed=97):
    """two segments with real DNA across the cut: the golden record with a gene, placed so that the cut (the middle tile) falls
    inside it; `gene_cut(m)` is the first base of the second segment"""
    gene = [s for n, s in golden_inputs() if n == "multigc_gene"][0]
    cut = gene_cut(m)
    rng = random.Random(seed)
    left = "".join(rng.choice("ACGT") for _ in range(cut - len(gene) // 2))
    right = "".join(rng.choice("ACGT") for _ in range(2 * cut - len(left) - len(gene)))
    return left + gene + right


def gene_cut(m):
    return 5 * check_tiles(m) * 64


def twin_want(m, cfg, seq):
    """helpers.TwinTies of one record (rc, lnv, path, V, counts(eps)): the oracle twin, once per record"""
    return ties_twin(m, cfg, seq)


def twin_path(T):
    return [(bg, en, s) for bg, en, s, _ in T.path]


_emu_seg = None


def emu_seg():
    global _emu_seg
    if _emu_seg is None:
        _emu_seg = ctypes.CDLL(SEG_EMU_LIB)
        _emu_seg.emu_dense_seg.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _emu_seg.emu_dense_seg_info.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p]
        _emu_seg.emu_dense_seg_apply.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return _emu_seg


def emu_seg_decode(m, seqs, slots=256):
    """the dense passes over the plan of `seqs` on the emulator: [(status, score, path, cells with the offsets applied, near ties)]
    and the plan {"segs", "seg_stop", "seg_stop2", "seg_status", "check_tiles"}"""
    E = emu_seg()
    assert E.emu_dense_seg(m.tables_ptr, slots) == 0
    try:
        res = emu_decode(m.tables_ptr, seqs, m.n_states, cells=True, lib=SEG_EMU_LIB)
        ties = emu_near_ties(len(seqs), lib=SEG_EMU_LIB)
        ck = ctypes.c_int()
        n = E.emu_dense_seg_info(None, None, None, None, 0, ctypes.byref(ck))
        segs = np.zeros((n, 5), dtype=np.int32)
        stop, stop2, status = (np.zeros(n, dtype=np.int32) for _ in range(3))
        E.emu_dense_seg_info(segs.ctypes.data, stop.ctypes.data, stop2.ctypes.data, status.ctypes.data, n, None)
        out = []
        for p, (st, lnv, path, V, _) in enumerate(res):
            V = np.ascontiguousarray(V)
            assert E.emu_dense_seg_apply(p, V.ctypes.data, V.shape[0], V.shape[1]) == 0
            out.append((st, lnv, path, V, ties[p]))
    finally:
        E.emu_dense_seg(None, 0)
    return out, {"segs": segs, "seg_stop": stop, "seg_stop2": stop2, "seg_status": status, "check_tiles": ck.value}


def gave_up(plan):
    return [int(q) for q in range(len(plan["segs"])) if plan["segs"][q][1] > 0 and plan["seg_stop"][q] <= -2]


def converged(plan):
    return [int(q) for q in range(len(plan["segs"])) if plan["segs"][q][1] > 0 and plan["seg_stop"][q] >= plan["segs"][q][2]]
