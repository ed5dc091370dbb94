"""The prefix scans of the preparation stage (decoder.hip: kSiteScan*, kFxScan*, kChunkOffsets) on pieces around the sizes of their
blocks, array by array against the emulator with no tolerance, on the first and on the second decode of a batch.

The content scans read their terms from tables converted to fixed point once per decoder, one record per pattern (kernels.h: FxTabs,
k1FxTermsRec); the emulator converts every term from the double tables (k1FxTermsCalc).  One batch per model:
- random DNA with lower-case stretches (the soft-masking bonus is added before the conversion) of 255-258, 511-514, 767-770,
  1 022-1 026 and 2 046-2 050 bases, in shuffled order: a piece ends a few slots before, on and after the edge of a scan block, and
  the block next to it belongs to another piece;
- two records whose GC content steps every few kb: several planes.
Models: human (two classes, soft-masking), nasonia (five classes), tetrahymena (intron content of order 3 beside exon content of order
4: the intron terms take patterns of their own; the 47-state trellis path takes it)."""
import random

import pytest

pytestmark = pytest.mark.gpu

import augustus_amd as ax
from helpers import *

LENS = [n for a, b in ((255, 258), (511, 514), (767, 770), (1022, 1026), (2046, 2050)) for n in range(a, b + 1)]
CFGS = {"human": ("human", {}), "nasonia": MORE_CFGS["nasonia"], "tetrahymena": ("tetrahymena", {})}


@pytest.fixture(autouse=True)
def _one_class_per_end_base(monkeypatch):
    """as in test_gpu_prep.py: the cache replays, which rewrite site values after the preparation stage, do not run"""
    monkeypatch.setenv("AUGX_EXACT_MULTICLASS", "0")
    monkeypatch.delenv("AUGX_BLK", raising=False)


def _softmasked(n, seed):
    rng = random.Random(seed)
    s = list(random_dna(n, seed))
    for _ in range(1 + n // 300):
        a = rng.randrange(n)
        b = min(n, a + rng.randint(1, 200))
        s[a:b] = "".join(s[a:b]).lower()
    return "".join(s)


def _records():
    recs = [("soft_%d" % n, _softmasked(n, 9700 + n)) for n in LENS]
    random.Random(9700).shuffle(recs)
    return recs + gc_step_records(2, 9701)


@pytest.mark.parametrize("cfg", list(CFGS))
def test_gpu_scans_at_the_block_edges_equal_emulator(cfg):
    species, opts = CFGS[cfg]
    m = ax.Model(config_path(), species, **opts)
    recs = _records()
    assert scan_block() in (256, 512, 1024)  # (the lengths above lie around the multiples of every block size the layout admits)
    emu_decode(m.tables_ptr, [s for _, s in recs], m.n_states, prep=True)
    assert any(c.islower() for _, s in recs for c in s)
    if cfg != "tetrahymena":
        assert max(int(emu_prep(i, "nPlanes")) for i in range(len(recs))) > 1, "no record with several planes"
    d = ax.Decoder(m, 0)
    b = ax.Batch(d, [s for _, s in recs])
    for turn in ("first decode", "second decode"):
        b.decode()
        for i, (name, _) in enumerate(recs):
            want = prep_arrays(emu_prep, i, False)
            got = prep_arrays(b.prep, i, False)
            assert [(w, pl) for w, pl, _ in got] == [(w, pl) for w, pl, _ in want], (cfg, turn, name)
            for (which, pl, a), (_, _, e) in zip(got, want):
                diff = prep_first_diff(a, e)
                assert diff is None, "%s, %s: record %s (piece %d of %d), array %s, plane %d: %s" % (cfg, turn, name, i, len(recs), which, pl, diff)
    b.close()
    d.close()
