"""augustus_amd -- MI355X-native ab-initio GHMM Viterbi decode (AUGUSTUS hot path), Python binding.

A thin ctypes layer over the C ABI of ``libaugx.so`` (``include/augx.h``).  The decode itself runs in
hand-written HIP kernels (``augustus_amd/csrc/device``); this module only marshals buffers.  There is no CPU
decode path: creating a :class:`Decoder` without a HIP device raises :class:`AugxError`.

Mirrors the reference's call sequence for this path
(``Properties::init`` .. ``NAMGene()`` .. ``StateModel::readAllParameters()`` ..
``NAMGene::doViterbiPiecewise``; reference ``src/augustus.cc:111-176,420``).
"""
import ctypes
import sys
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AUGX_LIB") or os.path.join(_HERE, "libaugx.so")  # (AUGX_LIB: a developer build of the same library)

AUGX_E_ARG = -1
AUGX_E_NODEVICE = -3
AUGX_E_HIP = -4
AUGX_E_UNSUPPORTED = -5
AUGX_E_NOPATH = -6
AUGX_E_NOMEM = -7
AUGX_E_RANGE = -8


class AugxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("augx error %d: %s" % (code, msg))
        self.code = code


class _Piece(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_char_p), ("len", ctypes.c_int64), ("init_kind", ctypes.c_int32),
                ("term_kind", ctypes.c_int32)]


class _State(ctypes.Structure):
    _fields_ = [("begin", ctypes.c_int32), ("end", ctypes.c_int32), ("state", ctypes.c_int16),
                ("type", ctypes.c_int16)]


class _Path(ctypes.Structure):
    _fields_ = [("states", ctypes.POINTER(_State)), ("n_states", ctypes.c_int32), ("status", ctypes.c_int32),
                ("ln_viterbi", ctypes.c_double)]


_lib = None


def lib():
    """Load libaugx.so (built in-tree by ``__graft_entry__.build()``); fails loudly if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("augustus_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'`"
                              % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.augx_last_error.restype = ctypes.c_char_p
        L.augx_version.restype = ctypes.c_char_p
        L.augx_model_tables.restype = ctypes.c_void_p
        L.augx_model_tables.argtypes = [ctypes.c_void_p]
        L.augx_model_option.restype = ctypes.c_char_p
        L.augx_model_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        L.augx_model_segmentable.restype = ctypes.c_int
        L.augx_model_segmentable.argtypes = [ctypes.c_void_p]
        L.augx_model_layout.restype = ctypes.c_int
        L.augx_model_layout.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
        L.augx_model_destroy.argtypes = [ctypes.c_void_p]
        L.augx_device_count.restype = ctypes.c_int
        L.augx_partition_lpt.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.augx_decode_sharded.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.augx_decoder_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.augx_decoder_destroy.argtypes = [ctypes.c_void_p]
        L.augx_decoder_set_share.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.augx_decoder_set_exact.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.augx_decoder_batch_capacity.restype = ctypes.c_int64
        L.augx_decoder_batch_capacity.argtypes = [ctypes.c_void_p]
        L.augx_batch_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.augx_batch_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.augx_batch_sync.argtypes = [ctypes.c_void_p]
        L.augx_batch_paths.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.augx_batch_cells.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.augx_batch_prep.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                      ctypes.POINTER(ctypes.c_int64)]
        L.augx_batch_near_ties.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.augx_decoder_set_near_tie_eps.argtypes = [ctypes.c_void_p, ctypes.c_double]
        L.augx_batch_replay_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
        L.augx_batch_replay_patches.restype = L.augx_batch_replay_sites.restype = ctypes.c_int64
        L.augx_batch_replay_patches.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.augx_batch_replay_sites.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        L.augx_batch_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float),
                                           ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        _plan = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                 ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        L.augx_plan_segments.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + _plan
        L.augx_batch_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + _plan + [ctypes.c_void_p, ctypes.c_void_p]
        L.augx_batch_forward.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.augx_batch_forward_cells.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
        L.augx_batch_destroy.argtypes = [ctypes.c_void_p]
        L.augx_rand_create.restype = ctypes.c_void_p
        L.augx_rand_create.argtypes = [ctypes.c_uint]
        L.augx_rand_next.argtypes = [ctypes.c_void_p]
        L.augx_rand_destroy.argtypes = [ctypes.c_void_p]
        L.augx_batch_sample.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.augx_decode_sampled.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p]
        L.augx_format_gff_sampled.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64,
                                              ctypes.POINTER(ctypes.c_int)]
        L.augx_path_free.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise AugxError(rc, lib().augx_last_error().decode(errors="replace"))


class Model:
    """Species model = option store + flat ln tables (``augx_model_load``)."""

    def __init__(self, config_path, species, **opts):
        L = lib()
        self._h = ctypes.c_void_p()
        names = (ctypes.c_char_p * len(opts))(*[k.encode() for k in opts])
        vals = (ctypes.c_char_p * len(opts))(*[str(v).encode() for v in opts.values()])
        _check(L.augx_model_load(config_path.encode(), species.encode(), len(opts), names, vals, ctypes.byref(self._h)))
        self.species = species
        self.config_path = config_path

    @property
    def tables_ptr(self):
        return ctypes.c_void_p(lib().augx_model_tables(self._h))

    @property
    def n_states(self):
        return ctypes.cast(self.tables_ptr, ctypes.POINTER(ctypes.c_int32))[0]

    def option(self, name):
        v = lib().augx_model_option(self._h, name.encode())
        return None if v is None else v.decode()

    def layout(self):
        """(kernel family: "trellis" / "dense", block size, whether the initial exon candidates are in the late class of the dense kernels)
        as ``augx_model_layout`` gives them, no device needed; AugxError(AUGX_E_UNSUPPORTED) with the reason for a model the decoder refuses"""
        out = (ctypes.c_int32 * 3)()
        _check(lib().augx_model_layout(self.tables_ptr, out))
        return ("dense" if out[0] else "trellis", int(out[1]), bool(out[2]))

    def segmentable(self):
        """``augx_model_segmentable``: can pieces of this model be cut into segments, by whichever kernel family decodes it?  (Never:
        the models with two intergenic states, ``genemodel=atleastone`` / ``exactlyone``; the forward pass of any model)"""
        return bool(lib().augx_model_segmentable(self.tables_ptr))

    def close(self):
        if self._h:
            lib().augx_model_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        # (objects that live until the interpreter shuts down -- e.g. held by the traceback of a failed test -- are left to the
        #  operating system: by then the HIP runtime may have run its own exit handlers, and calling into it crashes)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


# arrays of the preparation stage that ``augx_batch_prep`` hands out (include/augx.h: AUGX_PREP_*):
# name -> (which, dtype, fields, layout).  "slots": every slot of the piece (its before-first slot, its bases, its pad slots), stored
# in chunks of 1024 slots, field-major inside a chunk; "bases": one record per base (gcRaw: per GC window); "piece": per-piece scalars
PREP_CHUNK = 1024
PREP_ARRAYS = {
    "code": (0, "u1", 1, "slots"), "cnt": (1, "u4", 11, "slots"), "nsm": (2, "u4", 6, "slots"), "gcRaw": (3, "u1", 1, "bases"),
    "gcPlane": (4, "u1", 1, "bases"), "fx": (5, "u8", 20, "slots"), "sig": (6, "f8", 10, "bases"), "gate": (7, "u8", 1, "bases"),
    "plsR": (8, "f8", 3, "bases"), "ufx": (9, "u8", 6, "slots"), "ucnt": (10, "u4", 4, "slots"), "cls": (11, "i4", 1, "piece"),
    "nPlanes": (12, "i4", 1, "piece"), "planeCls": (13, "i4", 16, "piece"), "listCnt": (14, "i4", 1, "piece"),
    # the back pointers of the chain states as the last decode left them (near-tie flag: bit 7 / bit 6); bpD has one byte per state of
    # the model: handed out flat, [bases * S]
    "bpChain": (15, "u1", 8, "bases"), "bpD": (16, "u1", 1, "bases"),
}


def prep_fetch(call, which, plane=0):
    """one array of the preparation stage through ``call(which, plane, out, cap_bytes, n_bytes) -> rc`` (augx_batch_prep, or the test
    emulator's export of the same shape): [slots, fields] / [bases, fields], one-dimensional for a single field, a scalar array for
    cls / nPlanes / listCnt"""
    import numpy as np
    idx, dt, nf, layout = PREP_ARRAYS[which]
    nb = ctypes.c_int64(0)
    rc = call(idx, plane, None, 0, ctypes.byref(nb))
    if rc != AUGX_E_ARG or nb.value <= 0:  # (a buffer that is too small is refused with the size wanted; anything else is the refusal itself)
        raise AugxError(rc, "no array %r, plane %d" % (which, plane))
    raw = np.empty(nb.value, dtype=np.uint8)
    rc = call(idx, plane, raw.ctypes.data_as(ctypes.c_void_p), nb.value, ctypes.byref(nb))
    if rc != 0:
        raise AugxError(rc, "array %r, plane %d" % (which, plane))
    a = raw.view(np.dtype(dt))
    if layout == "slots":
        a = a.reshape(-1, nf, PREP_CHUNK).transpose(0, 2, 1).reshape(-1, nf)
    elif layout == "bases":
        a = a.reshape(-1, nf)
    elif nf == 1:
        return a.reshape(())
    return np.ascontiguousarray(a.reshape(-1) if nf == 1 else a)


class DecodedPiece:
    __slots__ = ("status", "ln_viterbi", "states")

    def __init__(self, status, lnv, states):
        self.status, self.ln_viterbi, self.states = status, lnv, states  # states: [(begin, end, state, type)]


class Batch:
    """A batch of pieces resident in HBM (``augx_batch_create``); decode() may be repeated and timed."""

    def __init__(self, decoder, seqs, init_kind=0, term_kind=0):
        L = lib()
        self.decoder = decoder
        self.n = len(seqs)
        self._keep = [s if isinstance(s, bytes) else s.encode() for s in seqs]
        self.lens = [len(s) for s in self._keep]
        P = (_Piece * self.n)()
        iks = init_kind if isinstance(init_kind, (list, tuple)) else [init_kind] * self.n
        tks = term_kind if isinstance(term_kind, (list, tuple)) else [term_kind] * self.n
        for i, s in enumerate(self._keep):
            P[i].seq, P[i].len, P[i].init_kind, P[i].term_kind = s, len(s), iks[i], tks[i]
        self._h = ctypes.c_void_p()
        self._decoded = False
        _check(L.augx_batch_create(decoder._h, P, self.n, ctypes.byref(self._h)))
        decoder._batches.add(self._h.value)   # (a decoder destroys its live batches before it goes: they hold a pointer to it)

    def decode(self, sync=True):
        _check(lib().augx_batch_decode(self.decoder._h, self._h))
        self._decoded = True
        if sync:
            _check(lib().augx_batch_sync(self.decoder._h))

    def kernel_ms(self):
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _check(lib().augx_batch_kernel_ms(self.decoder._h, self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"prep_ms": a.value, "trellis_ms": b.value, "backtrace_ms": c.value}

    def paths(self):
        L = lib()
        out = (_Path * self.n)()
        _check(L.augx_batch_paths(self.decoder._h, self._h, out))
        res = []
        for i in range(self.n):
            st = [(out[i].states[k].begin, out[i].states[k].end, out[i].states[k].state, out[i].states[k].type)
                  for k in range(out[i].n_states)]
            res.append(DecodedPiece(out[i].status, out[i].ln_viterbi, st))
            L.augx_path_free(ctypes.byref(out[i]))
        return res

    def cells(self, piece):
        import numpy as np
        S = self.decoder.model.n_states
        V = np.empty((self.lens[piece], S), dtype=np.float64)
        _check(lib().augx_batch_cells(self.decoder._h, self._h, piece, V.ctypes.data_as(ctypes.c_void_p)))
        return V

    def prep(self, piece, which, plane=0):
        """test hook (``augx_batch_prep``): array ``which`` (a name of PREP_ARRAYS) of one piece as the preparation stage of the last
        decode left it, plane ``plane`` of the arrays that have one per GC class of the piece (fx, plsR)"""
        L = lib()
        return prep_fetch(lambda w, pl, out, cap, nb: L.augx_batch_prep(self.decoder._h, self._h, piece, w, pl, out, cap, nb), which, plane)

    def near_ties(self):
        """test hook (``augx_batch_near_ties``): the near ties the back-trace of the last decode counted on the path of every piece"""
        import numpy as np
        out = np.zeros(self.n, dtype=np.int32)
        _check(lib().augx_batch_near_ties(self.decoder._h, self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return [int(x) for x in out]

    def replay_hooks(self):
        """test hooks (``augx_batch_replay_counters`` / ``_patches`` / ``_sites``; decoder created with AUGX_DEBUG_CELLS=1): three callables
        of the shape of the test emulator's exports, bound to this batch.  A refusal raises."""
        L, dh, bh = lib(), self.decoder._h, self._h

        def checked(f):
            def g(*a):
                r = f(dh, bh, *a)
                if r < 0:
                    _check(r)
                return r
            return g
        return checked(L.augx_batch_replay_counters), checked(L.augx_batch_replay_patches), checked(L.augx_batch_replay_sites)

    def plan(self):
        """``augx_batch_plan``: the plan of the trellis passes this batch was created with (see :func:`plan_segments`) and, once it has
        been decoded, ``seg_stop`` / ``seg_stop2``: where the fix-up of every segment and its continuation stopped (None before)"""
        L = lib()
        if not self._decoded:
            return _plan_query(lambda *a: L.augx_batch_plan(self.decoder._h, self._h, *a, None, None))
        return _plan_query(lambda *a: L.augx_batch_plan(self.decoder._h, self._h, *a), stops=True)

    def forward(self):
        """run the forward algorithm on the decoded batch (``augx_batch_forward``)"""
        _check(lib().augx_batch_forward(self.decoder._h, self._h))

    def forward_cells(self, piece):
        """(ln F matrix [len, S], ln P(sequence)) of one piece"""
        import numpy as np
        S = self.decoder.model.n_states
        F = np.empty((self.lens[piece], S), dtype=np.float64)
        lnp = ctypes.c_double()
        _check(lib().augx_batch_forward_cells(self.decoder._h, self._h, piece, F.ctypes.data_as(ctypes.c_void_p), ctypes.byref(lnp)))
        return F, lnp.value

    def sample(self, piece, n, rand):
        """n state paths of one piece sampled from the forward matrix (``augx_batch_sample``; run forward() first); the draws
        come from ``rand`` (a Rand: glibc's rand() restated, one stream over a run).  Returns [[(begin, end, state, type)]]"""
        L = lib()
        out = (_Path * max(1, n))()
        _check(L.augx_batch_sample(self.decoder._h, self._h, piece, n, rand._h, out))
        res = []
        for i in range(n):
            if out[i].status != 0:
                raise AugxError(out[i].status, "sampling failed")
            res.append([(out[i].states[k].begin, out[i].states[k].end, out[i].states[k].state, out[i].states[k].type)
                        for k in range(out[i].n_states)])
            L.augx_path_free(ctypes.byref(out[i]))
        return res

    def close(self):
        if self._h:
            if self._h.value in self.decoder._batches:  # (else the decoder has gone and has taken this batch with it)
                self.decoder._batches.discard(self._h.value)
                lib().augx_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        # (objects that live until the interpreter shuts down -- e.g. held by the traceback of a failed test -- are left to the
        #  operating system: by then the HIP runtime may have run its own exit handlers, and calling into it crashes)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Rand:
    """glibc's rand() after srand(seed), restated (``augx_rand``): the generator the reference samples with (never seeded: 1)."""

    def __init__(self, seed=1):
        self._h = ctypes.c_void_p(lib().augx_rand_create(seed))

    def next(self):
        return lib().augx_rand_next(self._h)

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            if self._h:
                lib().augx_rand_destroy(self._h)
                self._h = None
        except Exception:
            pass


def tss0(model, seq):
    """``augx_tss0``: (forward, reverse) ln value of the TSS window that begins at base 0 of `seq` -- what a later sequence of the same
    length is decoded with by the reference (include/augx.h)"""
    L = lib()
    L.augx_tss0.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
    b = seq if isinstance(seq, bytes) else seq.encode()
    out = (ctypes.c_double * 2)()
    _check(L.augx_tss0(model._h, b, len(b), out))
    return (out[0], out[1])


def decode_sampled(decoders, seqs, n_samples, rand, init_kind=0, term_kind=0):
    """``augx_decode_sampled``: Viterbi path + n_samples sampled paths per piece, batches in input order over the decoders.
    Returns [(DecodedPiece, [sampled paths])]."""
    L = lib()
    n = len(seqs)
    keep = [s if isinstance(s, bytes) else s.encode() for s in seqs]
    P = (_Piece * n)()
    iks = init_kind if isinstance(init_kind, (list, tuple)) else [init_kind] * n
    tks = term_kind if isinstance(term_kind, (list, tuple)) else [term_kind] * n
    for i, s in enumerate(keep):
        P[i].seq, P[i].len, P[i].init_kind, P[i].term_kind = s, len(s), iks[i], tks[i]
    D = (ctypes.c_void_p * len(decoders))(*[d._h for d in decoders])
    out = (_Path * n)()
    smp = (_Path * max(1, n * n_samples))()
    _check(L.augx_decode_sampled(D, len(decoders), P, n, n_samples, rand._h, out, smp))
    res = []
    for i in range(n):
        st = [(out[i].states[k].begin, out[i].states[k].end, out[i].states[k].state, out[i].states[k].type) for k in range(out[i].n_states)]
        sm = []
        for q in range(n_samples):
            sp = smp[i * n_samples + q]
            sm.append([(sp.states[k].begin, sp.states[k].end, sp.states[k].state, sp.states[k].type) for k in range(sp.n_states)])
            L.augx_path_free(ctypes.byref(sp))
        res.append((DecodedPiece(out[i].status, out[i].ln_viterbi, st), sm))
        L.augx_path_free(ctypes.byref(out[i]))
    return res


class _Cut(ctypes.Structure):
    _fields_ = [("record", ctypes.c_int32), ("status", ctypes.c_int32), ("begin", ctypes.c_int64), ("end", ctypes.c_int64),
                ("init_kind", ctypes.c_int32), ("term_kind", ctypes.c_int32)]


class _CutStats(ctypes.Structure):
    _fields_ = [("scout_tiles", ctypes.c_int32), ("batches", ctypes.c_int32), ("windows_decoded", ctypes.c_int32), ("windows_used", ctypes.c_int32)]


DECODE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(_Piece), ctypes.c_int, ctypes.POINTER(_Path))


def find_cuts(model, seqs, decode_fn, scout=-1):
    """``augx_find_cuts``: the pieces [(record, status, begin, end, init_kind, term_kind)] the records are cut into, the exam windows
    decoded through ``decode_fn(user, pieces, n, out_paths) -> rc`` (a DECODE_FN); also returns the statistics of the run."""
    L = lib()
    L.augx_find_cuts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64), DECODE_FN, ctypes.c_void_p,
                                 ctypes.c_int, ctypes.POINTER(ctypes.POINTER(_Cut)), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_CutStats)]
    L.augx_cuts_free.argtypes = [ctypes.POINTER(_Cut)]
    keep = [s.encode() if isinstance(s, str) else s for s in seqs]
    n = len(keep)
    c_seqs = (ctypes.c_char_p * n)(*keep)
    c_lens = (ctypes.c_int64 * n)(*[len(s) for s in keep])
    out = ctypes.POINTER(_Cut)()
    n_out = ctypes.c_int()
    st = _CutStats()
    _check(L.augx_find_cuts(model._h, n, c_seqs, c_lens, decode_fn, None, scout, ctypes.byref(out), ctypes.byref(n_out), ctypes.byref(st)))
    res = [(out[i].record, out[i].status, out[i].begin, out[i].end, out[i].init_kind, out[i].term_kind) for i in range(n_out.value)]
    L.augx_cuts_free(out)
    return res, {"scout_tiles": st.scout_tiles, "batches": st.batches, "windows_decoded": st.windows_decoded, "windows_used": st.windows_used}


def device_count():
    return lib().augx_device_count()


def _plan_query(call, stops=False):
    import numpy as np
    ns, nr, ck = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    est = np.zeros(2, dtype=np.int64)
    _check(call(None, 0, ctypes.byref(ns), None, 0, ctypes.byref(nr), ctypes.byref(ck), est.ctypes.data_as(ctypes.c_void_p), *((None, None) if stops else ())))
    segs = np.zeros((ns.value, 5), dtype=np.int32)
    runs = np.zeros(nr.value + 1, dtype=np.int32)
    more = ()
    if stops:
        more = (np.full(ns.value, -1, dtype=np.int32), np.full(ns.value, -1, dtype=np.int32))
    _check(call(segs.ctypes.data_as(ctypes.c_void_p), ns.value, ctypes.byref(ns), runs.ctypes.data_as(ctypes.c_void_p), nr.value, ctypes.byref(nr),
                ctypes.byref(ck), est.ctypes.data_as(ctypes.c_void_p), *[None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in more]))
    res = {"segs": segs, "run_seg0": runs[:nr.value + 1] if nr.value else runs[:0], "n_runs": nr.value, "check_tiles": ck.value,
           "est_tiles": int(est[0]), "est_per_piece": int(est[1])}
    res["seg_stop"], res["seg_stop2"] = more if stops else (None, None)
    return res


def plan_segments(model, lens, slots):
    """``augx_plan_segments`` (host only): the plan of the trellis passes for pieces of these lengths on ``slots`` workgroups.
    ``segs``: one row (piece, k, t0, t1, tlim) per segment, in tiles of 64 bases; ``run_seg0``: run r of pass 1 is the segments
    run_seg0[r] .. run_seg0[r + 1] - 1 (empty: one workgroup per segment); ``est_tiles`` / ``est_per_piece``: the estimate the plan was
    chosen by and that of the best plan that cuts every piece on its own"""
    import numpy as np
    a = np.ascontiguousarray(lens, dtype=np.int64)
    L = lib()
    return _plan_query(lambda *args: L.augx_plan_segments(model.tables_ptr, a.ctypes.data_as(ctypes.c_void_p), len(a), slots, *args))


def partition_lpt(lens, n_bins):
    """Longest-first bin packing used by decode_sharded (host only)."""
    import numpy as np
    a = np.asarray(lens, dtype=np.int64)
    out = np.zeros(len(a), dtype=np.int32)
    _check(lib().augx_partition_lpt(a.ctypes.data_as(ctypes.c_void_p), len(a), n_bins, out.ctypes.data_as(ctypes.c_void_p)))
    return out.tolist()


def decode_sharded(decoders, seqs, init_kind=0, term_kind=0):
    """``augx_decode_sharded``: pieces fanned over several decoders (one per GPU), results in input order."""
    L = lib()
    n = len(seqs)
    keep = [s if isinstance(s, bytes) else s.encode() for s in seqs]
    P = (_Piece * n)()
    iks = init_kind if isinstance(init_kind, (list, tuple)) else [init_kind] * n
    tks = term_kind if isinstance(term_kind, (list, tuple)) else [term_kind] * n
    for i, s in enumerate(keep):
        P[i].seq, P[i].len, P[i].init_kind, P[i].term_kind = s, len(s), iks[i], tks[i]
    D = (ctypes.c_void_p * len(decoders))(*[d._h for d in decoders])
    out = (_Path * n)()
    _check(L.augx_decode_sharded(D, len(decoders), P, n, out))
    res = []
    for i in range(n):
        st = [(out[i].states[k].begin, out[i].states[k].end, out[i].states[k].state, out[i].states[k].type)
              for k in range(out[i].n_states)]
        res.append(DecodedPiece(out[i].status, out[i].ln_viterbi, st))
        L.augx_path_free(ctypes.byref(out[i]))
    return res


class Decoder:
    """Device context (``augx_decoder_create``).  Raises AugxError(AUGX_E_NODEVICE) without a HIP device."""

    def __init__(self, model, device=0):
        self.model = model
        # handles of the live batches.  (Not weak references to the Batch objects: when a decoder and its batches become garbage together
        # -- held by the traceback of a failed test, say -- the collector clears weak references BEFORE it runs any __del__, the decoder
        # found no batch to close, went, and the batches' own __del__ then reached through their pointer to it)
        self._batches = set()
        self._h = ctypes.c_void_p()
        _check(lib().augx_decoder_create(model._h, device, ctypes.byref(self._h)))

    def set_exact(self, on=True):
        """``augx_decoder_set_exact``: replay the reference's snippet cache on pieces with several GC classes for the Viterbi run, too"""
        _check(lib().augx_decoder_set_exact(self._h, 1 if on else 0))

    def count_near_ties(self, on=True):
        """``augx_decoder_count_near_ties``: batches created from now on count the near ties on their chosen paths"""
        _check(lib().augx_decoder_count_near_ties(self._h, 1 if on else 0))

    def set_near_tie_eps(self, eps):
        """``augx_decoder_set_near_tie_eps``: batches created from now on flag and count near ties by this threshold (2e-7 by default)"""
        _check(lib().augx_decoder_set_near_tie_eps(self._h, float(eps)))

    def near_ties(self):
        """``augx_decoder_near_ties``: (cells, pieces) summed over the paths fetched so far"""
        L = lib()
        L.augx_decoder_near_ties.restype = ctypes.c_int64
        L.augx_decoder_near_ties.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        np_ = ctypes.c_int64()
        return int(L.augx_decoder_near_ties(self._h, ctypes.byref(np_))), int(np_.value)

    def set_share(self, n):
        """n decoders (streams) work on this device at the same time: plan the trellis segments for 1/n of its compute units"""
        _check(lib().augx_decoder_set_share(self._h, n))

    def decode(self, seqs, init_kind=0, term_kind=0):
        b = Batch(self, seqs, init_kind, term_kind)
        try:
            b.decode()
            return b.paths()
        finally:
            b.close()

    def close(self):
        if self._h:
            for h in list(self._batches):
                lib().augx_batch_destroy(ctypes.c_void_p(h))
            self._batches.clear()
            lib().augx_decoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        # (objects that live until the interpreter shuts down -- e.g. held by the traceback of a failed test -- are left to the
        #  operating system: by then the HIP runtime may have run its own exit handlers, and calling into it crashes)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------
# GenBank input and accuracy evaluation (host only; include/augx.h: augx_genbank_*, augx_eval_*)
# ---------------------------------------------------------------------------------------------------
INPUT_UNKNOWN, INPUT_GENBANK, INPUT_FASTA = 0, 1, 2
EXON_CDS, EXON_UTR5, EXON_UTR3 = 0, 1, 2


class _Exon(ctypes.Structure):
    _fields_ = [("begin", ctypes.c_int64), ("end", ctypes.c_int64), ("strand", ctypes.c_int32), ("frame", ctypes.c_int32), ("kind", ctypes.c_int32)]


class _Transcript(ctypes.Structure):
    _fields_ = [("gene_id", ctypes.c_char_p), ("transcript_id", ctypes.c_char_p), ("strand", ctypes.c_int32), ("complete", ctypes.c_int32),
                ("complete_left", ctypes.c_int32), ("complete_right", ctypes.c_int32), ("complete_5utr", ctypes.c_int32), ("complete_3utr", ctypes.c_int32),
                ("trans_start", ctypes.c_int64), ("trans_end", ctypes.c_int64), ("coding_start", ctypes.c_int64), ("coding_end", ctypes.c_int64),
                ("n_exons", ctypes.c_int32), ("exons", ctypes.POINTER(_Exon))]


class _PieceResult(ctypes.Structure):
    _fields_ = [("record", ctypes.c_int32), ("status", ctypes.c_int32), ("begin", ctypes.c_int64), ("end", ctypes.c_int64),
                ("states", ctypes.POINTER(_State)), ("n_states", ctypes.c_int32)]


_TX_FIELDS = ("gene_id", "transcript_id", "strand", "complete", "complete_left", "complete_right", "complete_5utr", "complete_3utr",
              "trans_start", "trans_end", "coding_start", "coding_end")


def _gb_lib():
    L = lib()
    if not getattr(L, "_gb_bound", False):
        L.augx_input_type.argtypes = [ctypes.c_char_p, ctypes.c_int64]
        L.augx_genbank_read.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.augx_genbank_read_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.augx_genbank_n_loci.argtypes = [ctypes.c_void_p]
        L.augx_genbank_messages.restype = ctypes.c_char_p
        L.augx_genbank_messages.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.augx_genbank_locus.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p),
                                         ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
        L.augx_genbank_transcript.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_Transcript)]
        L.augx_genbank_format_annotation.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64]
        L.augx_genbank_destroy.argtypes = [ctypes.c_void_p]
        L.augx_genbank_report.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_char_p, ctypes.c_int64]
        L.augx_eval_create.restype = ctypes.c_void_p
        L.augx_eval_add.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.augx_eval_print.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
        L.augx_eval_destroy.argtypes = [ctypes.c_void_p]
        L._gb_bound = True
    return L


def input_type(data):
    """FASTA, GenBank or neither (``augx_input_type``; reference ``GBSplitter::determineFileType``)."""
    if isinstance(data, str):
        data = data.encode()
    return _gb_lib().augx_input_type(data, len(data))


def _flat_transcripts(txs):
    """ctypes array of augx_transcript from dicts with the fields of _TX_FIELDS and "exons": [(begin, end, kind)]; the second value keeps the
    buffers alive"""
    arr = (_Transcript * max(1, len(txs)))()
    keep = []
    for i, t in enumerate(txs):
        ex = (_Exon * max(1, len(t["exons"])))()
        for k, e in enumerate(t["exons"]):
            ex[k].begin, ex[k].end, ex[k].kind = e[0], e[1], e[2]
            ex[k].strand, ex[k].frame = t["strand"], -1
        keep.append(ex)
        for f in _TX_FIELDS:
            v = t.get(f, None if f.endswith("_id") else -1 if f.endswith(("_start", "_end")) else 1)
            setattr(arr[i], f, v.encode() if isinstance(v, str) else v)
        arr[i].n_exons = len(t["exons"])
        arr[i].exons = ctypes.cast(ex, ctypes.POINTER(_Exon))
    return arr, keep


class GenBank:
    """The loci of a GenBank text with their annotated transcripts (``augx_genbank_read``; reference ``GBProcessor::getAnnoSequenceList``)."""

    def __init__(self, data, utr=False, stop_excluded=False, verbosity=3):
        L = _gb_lib()
        if isinstance(data, str):
            data = data.encode()
        self._h = ctypes.c_void_p()
        rc = L.augx_genbank_read(data, len(data), int(utr), int(stop_excluded), verbosity, ctypes.byref(self._h))
        self.stdout = L.augx_genbank_messages(self._h, 1).decode() if self._h else ""
        self.stderr = L.augx_genbank_messages(self._h, 2).decode() if self._h else ""
        if rc != 0:
            self.close()
            raise AugxError(rc, L.augx_last_error().decode(errors="replace") + ("\n" + self.stderr if self.stderr else ""))

    def __len__(self):
        return _gb_lib().augx_genbank_n_loci(self._h)

    def locus(self, i):
        """(name, sequence, length, [transcript dict])"""
        L = _gb_lib()
        name, seq, n, nt = ctypes.c_char_p(), ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int()
        _check(L.augx_genbank_locus(self._h, i, ctypes.byref(name), ctypes.byref(seq), ctypes.byref(n), ctypes.byref(nt)))
        txs = []
        for k in range(nt.value):
            t = _Transcript()
            _check(L.augx_genbank_transcript(self._h, i, k, ctypes.byref(t)))
            d = {f: getattr(t, f) for f in _TX_FIELDS}
            d["gene_id"], d["transcript_id"] = d["gene_id"].decode(), d["transcript_id"].decode()
            d["exons"] = [(t.exons[q].begin, t.exons[q].end, t.exons[q].kind, t.exons[q].strand, t.exons[q].frame) for q in range(t.n_exons)]
            txs.append(d)
        return name.value.decode(), seq.value.decode(), n.value, txs

    def annotation_gff(self, model, i):
        """the annotation of locus i as the reference prints it (``AnnoSequence::printGFF``), with the model's output options"""
        buf = ctypes.create_string_buffer(4 << 20)
        _check(_gb_lib().augx_genbank_format_annotation(model._h, self._h, i, buf, len(buf)))
        return buf.value.decode()

    def report(self, model, pieces, seconds=0.0):
        """the output of a run on this input from decoded pieces [(record, begin, end, status, [(begin, end, state, type)])]
        (``augx_genbank_report``; reference ``evaluateOnTestSet``)"""
        arr = (_PieceResult * max(1, len(pieces)))()
        keep = []
        for i, (rec, b, e, status, path) in enumerate(pieces):
            sts = (_State * max(1, len(path)))()
            for k, (pb, pe, s, ty) in enumerate(path):
                sts[k].begin, sts[k].end, sts[k].state, sts[k].type = pb, pe, s, ty
            keep.append(sts)
            arr[i].record, arr[i].status, arr[i].begin, arr[i].end, arr[i].n_states = rec, status, b, e, len(path)
            arr[i].states = ctypes.cast(sts, ctypes.POINTER(_State))
        buf = ctypes.create_string_buffer(16 << 20)
        _check(_gb_lib().augx_genbank_report(model._h, self._h, len(pieces), arr, seconds, buf, len(buf)))
        return buf.value.decode()

    def close(self):
        if self._h:
            _gb_lib().augx_genbank_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Evaluation:
    """Accuracy of predicted against annotated transcripts (``augx_eval_*``; reference ``Evaluation``)."""

    def __init__(self):
        self._h = ctypes.c_void_p(_gb_lib().augx_eval_create())

    def add(self, predicted, annotated, strand=0):
        """one locus; transcripts as the dicts of :meth:`GenBank.locus`; strand 0 = both, +1 / -1 = that strand only"""
        p, k1 = _flat_transcripts(predicted)
        a, k2 = _flat_transcripts(annotated)
        _check(_gb_lib().augx_eval_add(self._h, len(predicted), p, len(annotated), a, strand))

    def report(self):
        buf = ctypes.create_string_buffer(1 << 20)
        _check(_gb_lib().augx_eval_print(self._h, buf, len(buf)))
        return buf.value.decode()

    def __del__(self):
        if sys.is_finalizing():
            return
        try:
            if self._h:
                _gb_lib().augx_eval_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass
