// emu_dense_seg.cc -- the emulator with the dense kernels decoding in segments (dense.h: denseTiles): emu.cc as it is, plus an entry
// that makes every Viterbi run of a dense piece go through the passes of a plan -- pass 1 of every segment, the fix-ups, the
// continuation of the first one that gave up, segFinalizePiece -- so that emu_decode returns what the device returns for a cut batch:
// the stored cells (each region in its own frame), the score, the path of denseBacktracePiece over those regions, the near ties.
// The second run after the cache replays of a piece with several GC classes takes the same passes.
#include "emu.cc"

namespace {
struct DenseSegRun {
    const augx_tables *t = nullptr;
    int slots = 256;
    SegPlan plan;
    std::vector<int32_t> stop, stop2, status, covered, brkPos;
    std::vector<double> segD, segD2, brkOff;
    std::vector<int32_t> len;
} g_dsr;

template <int BLK> void denseSegPasses(const DevTables &T, const BatchView &B, DenseLds &L, int p) {
    const int s0 = B.pieceSeg0[p], s1 = B.pieceSeg0[p + 1];
    for (int q = s0; q < s1; q++) { B.segStop[q] = -1; B.segStop2[q] = -1; B.segStatus[q] = 0; }
    B.pieceCovered[p] = -1;
    for (int q = s0; q < s1; q++) denseTiles<BLK, 0, true, 1>(T, B, L, p, q);
    for (int q = s0; q < s1; q++) denseTiles<BLK, 0, true, 2>(T, B, L, p, q);
    denseTiles<BLK, 0, true, 3>(T, B, L, p, -1);
    segFinalizePiece(B, p);
}

bool denseSegHook(const DevTables &T, const BatchView &Bc, DenseLds &L, int p, int blk) {
    BatchView &B = const_cast<BatchView &>(Bc); // (the emulator's own view, a local of emu_decode_dense: the plan is entered once per decode)
    DenseSegRun &R = g_dsr;
    if (B.segs != R.plan.segs.data() || R.plan.segs.empty()) {
        const int n = B.nPieces;
        std::vector<augx_piece> pieces((size_t)n);
        for (int i = 0; i < n; i++) { pieces[i].seq = B.raw + B.off[i] + 1; pieces[i].len = B.len[i]; pieces[i].init_kind = B.initKind[i]; pieces[i].term_kind = B.termKind[i]; }
        BatchLayout Lay;
        Lay.build(pieces.data(), n);
        R.plan = planSegments(Lay, *R.t, R.slots, 0, pieces.data());
        const size_t nS = R.plan.segs.size();
        R.stop.assign(nS, -1); R.stop2.assign(nS, -1); R.status.assign(nS, 0); R.covered.assign((size_t)n, -1); R.brkPos.assign(nS, 0);
        R.segD.assign(nS, 0.0); R.segD2.assign(nS, 0.0); R.brkOff.assign(nS, 0.0);
        R.len.assign(B.len, B.len + n);
        B.nSegs = (int)nS; B.segs = R.plan.segs.data(); B.pieceSeg0 = R.plan.pieceSeg0.data();
        B.segCheckTiles = R.plan.checkTiles;
        if (const char *e = getenv("AUGX_SEG_CHECK_TILES")) B.segCheckTiles = atoi(e);
        B.segStop = R.stop.data(); B.segStop2 = R.stop2.data(); B.segStatus = R.status.data(); B.pieceCovered = R.covered.data();
        B.segD = R.segD.data(); B.segD2 = R.segD2.data(); B.brkPos = R.brkPos.data(); B.brkOff = R.brkOff.data();
    }
    if (blk == 8) denseSegPasses<8>(T, B, L, p); else if (blk == 4) denseSegPasses<4>(T, B, L, p); else denseSegPasses<2>(T, B, L, p);
    return true;
}
} // namespace

extern "C" {
// from now on emu_decode runs the Viterbi pass of a dense model over the plan planSegments makes for `slots` workgroups (AUGX_SEG_LEN
// and AUGX_SEG_CHECK_TILES apply as on the device); t == NULL: as emu.cc does
int emu_dense_seg(const augx_tables *t, int slots) {
    g_dsr.t = t; g_dsr.slots = slots > 0 ? slots : 1;
    g_dsr.plan = SegPlan();
    g_emuDenseSegHook = t ? denseSegHook : nullptr;
    return 0;
}
// the plan of the last decode and what its passes left: segs [n][5] as augx_plan_segments, seg_stop / seg_stop2 as augx_batch_plan
int emu_dense_seg_info(int32_t *segs, int32_t *seg_stop, int32_t *seg_stop2, int32_t *seg_status, int cap, int *check_tiles) {
    const SegPlan &P = g_dsr.plan;
    const int nS = (int)P.segs.size();
    if (check_tiles) *check_tiles = P.checkTiles;
    for (int q = 0; q < nS && q < cap; q++) {
        const SegDesc &sd = P.segs[(size_t)q];
        if (segs) { int32_t *o = segs + (size_t)q * 5; o[0] = sd.piece; o[1] = sd.k; o[2] = sd.t0; o[3] = sd.t1; o[4] = sd.tlim; }
        if (seg_stop) seg_stop[q] = g_dsr.stop[(size_t)q];
        if (seg_stop2) seg_stop2[q] = g_dsr.stop2[(size_t)q];
        if (seg_status) seg_status[q] = g_dsr.status[(size_t)q];
    }
    return nS;
}
// the stored cells of piece p of the last decode ([len][S], as emu_decode returned them) with the offset of every region applied,
// as augx_batch_cells does
int emu_dense_seg_apply(int p, double *V, int len, int S) {
    const SegPlan &P = g_dsr.plan;
    if (p < 0 || p + 1 >= (int)P.pieceSeg0.size() || len != g_dsr.len[(size_t)p]) return AUGX_E_ARG;
    const int s0 = P.pieceSeg0[(size_t)p], s1 = P.pieceSeg0[(size_t)p + 1];
    if (s1 - s0 <= 1) return 0;
    int r = s0;
    for (int q = 0; q < len; q++) {
        while (r + 1 < s1 && q > g_dsr.brkPos[(size_t)r]) r++;
        for (int s = 0; s < S; s++) V[(int64_t)q * S + s] = V[(int64_t)q * S + s] + g_dsr.brkOff[(size_t)r];
    }
    return 0;
}
}
