// The reference's content cache of the short-intron states, replayed -- host code shared by the device library and the lane-loop
// emulator.  Only pieces with several GC classes need it, and only with the forward algorithm / sampling on.
//
// A short intron (lessD state) ending at base j scores its interior with IntronModel::seqProb -> SnippetProbs::getSeqProb(right = j,
// len) (reference src/intronmodel.cc:1064-1067, src/statemodel.cc:312-342): a cache keyed by (end base, length) that is never
// emptied when the GC class changes (IntronModel::updateToLocalGC only swaps the emission table, src/intronmodel.cc:495-503).  A
// request is answered from the longest cached piece that fits plus a recursive request for the rest, and only what is not cached is
// computed -- with the table of the class current AT THAT TIME.  Within 2 d bases after a class step an interior may therefore
// be the product of chunks scored under different classes, which chunks depending on what was requested before: on which
// predecessor cells were alive (a request is only made for a live predecessor, src/intronmodel.cc:589-600) and in which order
// (base by base, lessD states in state order, predecessor positions from near to far).  The device scores the whole interior with
// the class of its end base; this replay finds, for every candidate in the window after a class step, the chunks the reference
// would have used, and the term of the candidate is rebuilt from them (fixed-point prefix differences per class: exact).
// What comes out are the forward values of the reference to 1e-9, hence its sampled paths.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <vector>
#include <algorithm>
#include <utility>
#include "dp.h"

namespace augx {
namespace dev {

struct MemoChunk { int32_t end, len; int32_t plane; };
struct MemoEntry { int32_t len; std::vector<MemoChunk> dec; };

// global index of the candidate record (as in blkOff) and its new term; the request it answers, relative to the piece: end base j,
// short-intron state s, predecessor end eop (tests compare rebuilt terms by this key: candidate space is handed out by atomic adds,
// so that a global index means nothing outside the run it comes from)
struct MemoPatch { uint64_t item; double te; int32_t j, s, eop; };

// which of its paths a replay took (plain adds, always compiled; tests/test_emu_replay.py proves that the test inputs reach them)
enum SnipCount {
    SC_WINDOWS, SC_MERGED, SC_MERGED_3STEPS, SC_CLAMP_START, SC_CLAMP_END, SC_MAX_BLOCKS /* a maximum */, SC_EMPTY_BLOCK_WINS, SC_PIECES_3WIN,
    SC_GET_EMPTY, SC_GET_EXTEND, SC_GET_HIT, SC_GET_NONE, SC_GET_PART,
    SC_ADD_SAME, SC_MAP_FALLBACK, SC_COL0_REQ, SC_BELOW_ROW0, SC_MIXED_SAME, SC_PATCH_FWD, SC_PATCH_REV, SC_WINS_3PLANES, SC_N
};
struct SnipCounters {
    long long c[SC_N] = {0};
    void add(const SnipCounters &o) { for (int i = 0; i < SC_N; i++) { if (i == SC_MAX_BLOCKS) c[i] = c[i] > o.c[i] ? c[i] : o.c[i]; else c[i] += o.c[i]; } }
};

// One window of a piece as the windowed mode fetches it: what kGatherWindows (decoder.hip) packs and where.  The window replays the
// bases t0..t1 (clamped to the piece); it reads the candidate records of the blocks b0..b1 (pool, from poolOff), the prefix slots
// g0 .. g0 + nSlots - 1 of every plane and strand (from fxOff, laid out [plane][strand][slot]) and the rows r0 .. r0 + nRows - 1 of
// the matrix (from fOff; none after a Viterbi run of the 47-state kernels, which keep no matrix).  r0 lies d + 2 before t0: a short
// intron that ends in the window begins at most d bases before it.
struct GatherWin { int64_t o, gb0, poolOff, fxOff, fOff; int32_t b0, b1, g0, nSlots, nPl, r0, nRows, pad; };
// the windows {t0, t1} of a piece of `len` bases (as run() hands them to prefetch) -> their GatherWin records; pool / fx / fr: the sizes of
// the three packed arrays (records, slots, doubles).  blkCnt: [nBlocks][2] of the piece; matrix: rows of a matrix are read
inline void planGatherWins(const std::vector<std::pair<int, int>> &tt, int len, int blk, int d, int nPl, const uint32_t *blkCnt, bool matrix, int S,
                           int64_t o, int64_t gb0, std::vector<GatherWin> &wins, int64_t &pool, int64_t &fx, int64_t &fr) {
    wins.clear();
    pool = 0; fx = 0; fr = 0;
    for (auto w : tt) {
        const int t0 = w.first < 0 ? 0 : w.first, t1 = w.second > len - 1 ? len - 1 : w.second;
        GatherWin g;
        memset(&g, 0, sizeof g);
        g.o = o; g.gb0 = gb0; g.b0 = t0 / blk; g.b1 = t1 / blk;
        g.r0 = t0 - d - 2 > 0 ? t0 - d - 2 : 0;
        g.g0 = g.r0; g.nSlots = t1 + 1 - g.r0 + 1; g.nPl = nPl;
        g.nRows = matrix ? t1 - g.r0 + 1 : 0;
        g.poolOff = pool; g.fxOff = fx; g.fOff = fr;
        for (int q = g.b0; q <= g.b1; q++) pool += blkCnt[(size_t)q * 2 + 1];
        fx += (int64_t)g.nPl * 2 * g.nSlots;
        fr += (int64_t)g.nRows * S;
        wins.push_back(g);
    }
}

// everything of one piece the replay reads (host memory)
struct SnippetReplay {
    const augx_tables *t = nullptr;
    int n = 0, S = 0, blk = 8, d = 0;
    bool dense = false;                   // the candidate records are those of the dense kernels (dense.h): the pair is (base of the block << 7) | state,
                                          // `src` names the predecessor state, a start from column 0 has predecessor end 0; aliveness from the dense matrix F
    // which predecessor cells are alive, from a first run: the ln forward matrix F [n][S], or -- after a Viterbi run, which keeps no
    // matrix -- the values the trellis left at the donor sites (ldVal / rdVal: [entry][3 frames]) and the initial column col0 [S]
    const double *F = nullptr;
    const double *ldVal = nullptr, *rdVal = nullptr, *col0 = nullptr;
    const uint8_t *plane = nullptr;       // [n] plane of every base
    const int32_t *planeCls = nullptr;    // [MAXPL] class of a plane
    int nPlanes = 1;
    Item *items = nullptr;                // candidates of the piece, starting at global index item0 (te is rewritten in place)
    uint64_t item0 = 0;
    // Windowed mode (the device library): only what a window reads is fetched from HBM, by `fetch`, before the window is replayed --
    // the candidate records of its blocks (pool / blkPool), the rows fRow0.. of F, the prefix slots fx0.. .  Whole mode (the
    // emulator, whose arrays are host memory anyway): fetch is empty, everything above points at the whole piece.
    std::function<int(int, int)> fetch;   // (t0, t1) -> 0, or an error code that run() hands on
    // (optional) told every window of the piece before the first one is replayed -- {t0, t1} in the order run() takes them --, so
    // that what they read can come from HBM in one go; fetch then only has to pick the window's part
    std::function<int(const std::vector<std::pair<int, int>> &)> prefetch;
    std::vector<Item> pool;
    std::vector<int64_t> blkPool;         // [nBlocks] first record of the block in pool, -1: not fetched
    const double *F0 = nullptr;           // row 0 of F (the initial column), windowed mode
    int fRow0 = 0, fx0 = 0;
    Item *blockItems(int b) { return fetch ? (blkPool[(size_t)b] >= 0 ? pool.data() + blkPool[(size_t)b] : nullptr) : items + (blkOff[(size_t)b * 2 + 1] - item0); }
    const uint64_t *blkOff = nullptr;     // [nBlocks][2]
    const uint32_t *blkCnt = nullptr;     // [nBlocks][2]
    // fixed-point content prefix of the intron model: fx(plane, rev, g) with g = slot relative to the piece (0 = before the first base)
    std::vector<std::vector<uint64_t>> fxF, fxR; // [plane][n + 1]
    std::vector<MemoPatch> patches;
    SnipCounters stats;

    int64_t segFx(int pl, bool rev, int l, int r) const { // fixed-point content of bases l..r under plane pl
        if (l > r) return 0;
        const std::vector<uint64_t> &a = rev ? fxR[pl] : fxF[pl];
        return (int64_t)(a[(size_t)(r + 1 - fx0)] - a[(size_t)(l - fx0)]);
    }

    // Windowed mode: the part of the packed arrays (planGatherWins; poolAll / fxAll / FAll: as kGatherWindows left them) that the next
    // window reads becomes pool / blkPool, fxF / fxR and F.  The windows are handed out in the order prefetch was told them: (ft0, ft1)
    // must be the one whose turn it is.  blkPool holds [nBlocks] entries, -1 before the first window; only the blocks of the window
    // before hold anything (a 2 Mbp piece has 250 000 blocks, a window 300).  Returns AUGX_OK, or AUGX_E_ARG for another window.
    int cutWindow(const std::vector<GatherWin> &wins, size_t &nextWin, int ft0, int ft1, const std::vector<Item> &poolAll,
                  const std::vector<uint64_t> &fxAll, const std::vector<double> &FAll, bool matrix) {
        if (nextWin >= wins.size()) return AUGX_E_ARG;
        const GatherWin &g = wins[nextWin++];
        {
            const int t0 = ft0 < 0 ? 0 : ft0, t1 = ft1 > n - 1 ? n - 1 : ft1;
            if (g.b0 != t0 / blk || g.b1 != t1 / blk || g.r0 != (t0 - d - 2 > 0 ? t0 - d - 2 : 0)) return AUGX_E_ARG;
        }
        if (nextWin >= 2) {
            const GatherWin &pw = wins[nextWin - 2];
            for (int q = pw.b0; q <= pw.b1; q++) blkPool[(size_t)q] = -1;
        }
        size_t total = 0;
        for (int q = g.b0; q <= g.b1; q++) {
            if (blkCnt[(size_t)q * 2 + 1]) blkPool[(size_t)q] = (int64_t)total;
            total += blkCnt[(size_t)q * 2 + 1];
        }
        pool.assign(poolAll.begin() + g.poolOff, poolAll.begin() + g.poolOff + (int64_t)total);
        pool.resize(total + 1);
        if (matrix) { F = FAll.data() + g.fOff; fRow0 = g.r0; }
        fx0 = g.r0;
        for (int pl = 0; pl < g.nPl; pl++)
            for (int rev = 0; rev < 2; rev++) {
                std::vector<uint64_t> &dst = rev ? fxR[pl] : fxF[pl];
                const uint64_t *src = fxAll.data() + g.fxOff + ((int64_t)pl * 2 + rev) * g.nSlots;
                dst.assign(src, src + g.nSlots);
            }
        return AUGX_OK;
    }

    // ---- the cache of one strand: lists[base] sorted by length (SnippetList).  The bases a window touches lie in [flatLo, flatLo + size):
    //      a vector indexed by base (round 6: the std::map it was cost a third of the replay); anything outside goes to the map
    std::map<int, std::vector<MemoEntry>> lists[2];
    std::vector<std::vector<MemoEntry>> flat[2];
    int flatLo = 0;
    std::vector<MemoEntry> *listAt(int st, int base, bool create) {
        const int64_t k = (int64_t)base - flatLo;
        if (k >= 0 && k < (int64_t)flat[st].size()) return &flat[st][(size_t)k];
        stats.c[SC_MAP_FALLBACK]++;
        if (create) return &lists[st][base];
        auto f = lists[st].find(base);
        return f == lists[st].end() ? nullptr : &f->second;
    }

    void add(int st, int base, int len, const std::vector<MemoChunk> &dec) { // SnippetProbs::addProb, src/statemodel.cc:344-370
        std::vector<MemoEntry> &v = *listAt(st, base, true);
        size_t pos = 0;
        while (pos < v.size() && v[pos].len < len) pos++;
        if (pos < v.size() && v[pos].len == len) { stats.c[SC_ADD_SAME]++; return; } // ("tried to add snippet of same length": the reference keeps the old one)
        v.insert(v.begin() + (long)pos, MemoEntry{len, dec});
    }
    std::vector<MemoChunk> get(int st, int base, int len, int curPlane) { // SnippetProbs::getSeqProb, src/statemodel.cc:312-342
        std::vector<MemoChunk> dec;
        if (len == 0) return dec;
        std::vector<MemoEntry> *fv = listAt(st, base, false);
        if (fv && !fv->empty()) {
            std::vector<MemoEntry> &v = *fv;
            if (v.back().len < len) {
                stats.c[SC_GET_EXTEND]++;
                const int l1 = v.back().len;
                const std::vector<MemoChunk> last = v.back().dec; // (copy: the recursion may add to other lists, not to this one)
                dec = get(st, base - l1, len - l1, curPlane);
                dec.insert(dec.end(), last.begin(), last.end());
                add(st, base, len, dec);
            } else { // SnippetList::getProb, src/statemodel.cc:378-393: the longest cached length <= len
                int partlen = 0;
                const std::vector<MemoChunk> *pd = nullptr;
                if (v.front().len <= len) {
                    size_t k = 0;
                    while (k + 1 < v.size() && v[k + 1].len < len) k++;
                    if (k + 1 < v.size() && v[k + 1].len == len) k++;
                    partlen = v[k].len;
                    pd = &v[k].dec;
                }
                if (partlen == len) { stats.c[SC_GET_HIT]++; dec = *pd; }
                else if (partlen == 0) {
                    stats.c[SC_GET_NONE]++;
                    dec.push_back({base, len, curPlane});
                    add(st, base, len, dec);
                } else {
                    stats.c[SC_GET_PART]++;
                    const std::vector<MemoChunk> part = *pd;
                    dec = get(st, base - partlen, len - partlen, curPlane);
                    dec.insert(dec.end(), part.begin(), part.end());
                }
            }
        } else {
            stats.c[SC_GET_EMPTY]++;
            dec.push_back({base, len, curPlane});
            add(st, base, len, dec);
        }
        return dec;
    }

    // replay the requests of the bases t0..t1 (lists empty at t0); candidates ending at or after `from` whose chunks are not all of
    // their own plane get a new term
    void window(int t0, int t1, int from) {
        lists[0].clear(); lists[1].clear();
        flatLo = t0 - d - 64;
        for (int st = 0; st < 2; st++) { flat[st].clear(); flat[st].resize((size_t)(t1 - flatLo + 2 > 0 ? t1 - flatLo + 2 : 0)); }
        const int S2 = S;
        std::vector<int> lessF, lessR;
        for (int s = 0; s < S2; s++) {
            if (t->state_kind[s] == AUGX_K_LESSD) lessF.push_back(s);
            else if (t->state_kind[s] == AUGX_K_RLESSD) lessR.push_back(s);
        }
        struct Req { int eop; Item *item; uint64_t gidx; };
        {   // (what the window is, for the counters)
            const int c1 = t1 < n - 1 ? t1 : n - 1;
            stats.c[SC_WINDOWS]++;
            if (t0 < 0) stats.c[SC_CLAMP_START]++;
            if (t1 > n - 1) stats.c[SC_CLAMP_END]++;
            const int nb = c1 / blk - (t0 < 0 ? 0 : t0) / blk + 1;
            if (nb > stats.c[SC_MAX_BLOCKS]) stats.c[SC_MAX_BLOCKS] = nb;
            bool emptyBlock = false;
            for (int q = (t0 < 0 ? 0 : t0) / blk; q <= c1 / blk; q++) emptyBlock = emptyBlock || blkCnt[(size_t)q * 2 + 1] == 0;
            if (emptyBlock) stats.c[SC_EMPTY_BLOCK_WINS]++;
            unsigned seen = 0;
            for (int q = t0 - d - 2 > 0 ? t0 - d - 2 : 0; q <= c1; q++) seen |= 1u << plane[q];
            int np = 0;
            for (; seen; seen &= seen - 1) np++;
            if (np >= 3) stats.c[SC_WINS_3PLANES]++;
        }
        std::vector<Req> reqs;
        // the candidates of a block, ordered by their (base, state) pair once per block (round 6: every one of the block's 8 x 6
        // (base, short-intron state) pairs went through all of the block's ~120 records)
        std::vector<uint32_t> byPair, pairFirst;
        int bucketBlock = -1;
        const int pidBits = dense ? 7 : 6, nPid = blk << pidBits;
        for (int j = (t0 < 1 ? 1 : t0); j <= t1 && j < n; j++) {
            const int pl = plane[j];
            const int b = j / blk;
            Item *bi = blockItems(b);
            const uint32_t cnt = bi ? blkCnt[(size_t)b * 2 + 1] : 0;
            if (b != bucketBlock) {
                bucketBlock = b;
                pairFirst.assign((size_t)nPid + 1, 0);
                for (uint32_t it = 0; it < cnt; it++) { const uint32_t pid = bi[it].kp >> KEY_BITS; if (pid < (uint32_t)nPid) pairFirst[(size_t)pid + 1]++; }
                for (int q = 0; q < nPid; q++) pairFirst[(size_t)q + 1] += pairFirst[(size_t)q];
                byPair.resize(cnt);
                std::vector<uint32_t> w(pairFirst.begin(), pairFirst.end() - 1);
                for (uint32_t it = 0; it < cnt; it++) { const uint32_t pid = bi[it].kp >> KEY_BITS; if (pid < (uint32_t)nPid) byPair[w[(size_t)pid]++] = it; }
            }
            for (int st = 0; st < 2; st++) {
                const std::vector<int> &states = st == 0 ? lessF : lessR;
                for (int s : states) {
                    const uint32_t pid = dense ? (uint32_t)(((j % blk) << 7) | s) : (uint32_t)(((j % blk) << 6) | s);
                    const int a = t->anc[s][0];
                    reqs.clear();
                    for (uint32_t bq = pairFirst[(size_t)pid]; bq < pairFirst[(size_t)pid + 1]; bq++) {
                        const uint32_t it = byPair[bq];
                        const Item &I = bi[it];
                        if ((I.kp >> KEY_BITS) != pid || !(I.te > -INFINITY)) continue;
                        const int eop = (int)(I.kp & KEY_MASK) - KEY_BIAS;
                        const uint32_t tag = dense ? (eop <= 0 ? SRC_COL0 : SRC_LIST) : I.src >> 30;
                        // (a request is made only where a predecessor cell is alive; column 0 holds the initial probabilities)
                        double pv;
                        if (tag == SRC_COL0) stats.c[SC_COL0_REQ]++;
                        else if (fetch && (dense || F) && eop < fRow0) stats.c[SC_BELOW_ROW0]++;
                        if (dense) pv = eop <= 0 ? (F0 ? F0 : F)[(size_t)(I.src & 127u)] : (eop >= fRow0 ? F[(size_t)(eop - fRow0) * S2 + (I.src & 127u)] : -INFINITY);
                        else if (F) pv = tag == SRC_COL0 ? (F0 ? F0 : F)[(size_t)(I.src & 0x3Fu)] : (eop >= fRow0 ? F[(size_t)(eop - fRow0) * S2 + a] : -INFINITY);
                        else if (tag == SRC_COL0) pv = col0[I.src & 0x3Fu];
                        else pv = (((I.src >> 26) & 3) == 2 ? ldVal : rdVal)[(size_t)(I.src & 0xFFFFFFu) * 3 + ((I.src >> 24) & 3)];
                        if (!(pv > -INFINITY)) continue;
                        reqs.push_back({tag == SRC_COL0 ? 0 : eop, bi + it, blkOff[(size_t)b * 2 + 1] + it});
                    }
                    std::sort(reqs.begin(), reqs.end(), [](const Req &x, const Req &y) { return x.eop > y.eop; }); // from near to far
                    for (const Req &rq : reqs) {
                        const int len = j - rq.eop; // bases eop + 1 .. j
                        const std::vector<MemoChunk> dec = get(st, j, len, pl);
                        if (j < from) continue;
                        bool mixed = false;
                        for (const MemoChunk &c : dec) mixed = mixed || c.plane != pl;
                        if (!mixed) continue;
                        int64_t fx = 0;
                        for (const MemoChunk &c : dec) fx += segFx(c.plane, st == 1, c.end - c.len + 1, c.end);
                        // the term as K2a builds it (kernels.h: varEvalItem): transition + (length + content)
                        const bool fwd = st == 0;
                        const int begin = rq.eop + 1;
                        const int bobi = fwd ? begin - t->De - 2 : begin - (t->U + t->As + 2);
                        const int eobi = fwd ? j + t->U + t->As + 2 : j + t->De + 2;
                        int intronLength = eobi - bobi + 1;
                        if (intronLength > t->d || intronLength < 0) intronLength = 0;
                        const int cls = planeCls[pl];
                        const double tr = t->ln_trans[((int64_t)cls * S2 + a) * S2 + s];
                        const double te = tr + (t->len_intron[intronLength] + (double)fx * AUGX_FX_INV);
                        if (te != rq.item->te) { rq.item->te = te; patches.push_back({rq.gidx, te, j, s, rq.eop}); stats.c[fwd ? SC_PATCH_FWD : SC_PATCH_REV]++; }
                        else stats.c[SC_MIXED_SAME]++;
                    }
                }
            }
        }
    }

    // all windows of the piece: a class step at base b can leave its mark on candidates ending in [b, b + 2 d]; the caches that
    // matter then were started no earlier than b - d
    int run() {
        patches.clear();
        stats = SnipCounters(); // (as AssMemoReplay::run: the counts of this run alone)
        if (nPlanes <= 1) return 0;
        std::vector<int> steps;
        for (int j = 1; j < n; j++)
            if (plane[j] != plane[j - 1]) steps.push_back(j);
        std::vector<std::pair<int, int>> wins; // {first step, t1} of every window
        for (size_t i = 0; i < steps.size();) {
            const int first = steps[i];
            int t1 = first + 2 * d + 64;
            size_t k = i + 1;
            while (k < steps.size() && steps[k] - d - 64 <= t1) { t1 = steps[k] + 2 * d + 64; k++; }
            wins.push_back({first, t1});
            if (k - i >= 2) stats.c[SC_MERGED]++;
            if (k - i >= 3) stats.c[SC_MERGED_3STEPS]++;
            i = k;
        }
        if (wins.size() >= 3) stats.c[SC_PIECES_3WIN]++;
        if (prefetch) {
            std::vector<std::pair<int, int>> tt;
            for (auto &w : wins) tt.push_back({w.first - d - 64, w.second});
            const int rc = prefetch(tt);
            if (rc) return rc;
        }
        for (auto &w : wins) {
            if (fetch) { const int rc = fetch(w.first - d - 64, w.second); if (rc) return rc; }
            window(w.first - d - 64, w.second, w.first);
        }
        return 0;
    }
};

} // namespace dev
} // namespace augx
