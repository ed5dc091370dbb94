// k_trellis.hip -- the trellis kernels of one block size (AUGX_TU_BLK): pass 1 (MODE 0), fix-ups (1), continuation (2, 3), each
// also as the build whose chain wavefront flags near ties.  Body: kernels.h: trellisPiece.
#include "kernels.h"
#include "launch.h"

using namespace augx;
using namespace augx::dev;

// MODE 0: pass 1, one workgroup per segment (= per piece when no piece is cut), or per run of segments (RUNS); 1: the fix-ups; 2: continuation of pieces whose
// fix-up gave up, one workgroup per piece (kernels.h: trellisPiece).
// The default build (no near-tie flags) is ROLE-SPECIALISED: every wavefront of the workgroup branches once, on its (scalar)
// index, into the instantiation of trellisPiece that carries its own role's constants only -- 203 instead of 256 VGPRs and no
// scratch for <8, 0> (profiles/EXPERIMENTS.md, round 4/5).
// INVARIANT the switch rests on: the workgroup barriers of trellisPiece (BLOCK_SYNC / __syncthreads -> s_barrier) then sit in
// wave-divergent control flow, outside HIP's barrier contract; on s_barrier hardware it is sound exactly while all eight
// instantiations execute the SAME NUMBER of barriers -- every barrier of trellisPiece is reached by every wavefront, none stands
// under a condition that depends on the wavefront's index (role work between two barriers is guarded per role, the barriers are
// not).  The sequential emulator cannot see a violation; tests/test_gpu_parity.py::test_gpu_role_specialised_equals_common_body
// compares this build with the common-body (TIES) build cell for cell on the device.
// RUNS (pass 1 when the plan has runs, layout.h: SegPlan::runSeg0; a kernel of its own, so that the one-segment kernels stay as they
// are): workgroup r does the segments of run r one after the other.  The barrier between two segments stands OUTSIDE the role
// switch, so every wavefront executes it once per segment whatever its role: the next segment re-initialises LDS that another
// wavefront may still be reading.  Every early return of trellisPiece (a piece with several classes that this version does not
// decode, a piece without a nucleotide) depends on the segment alone and comes before its first barrier: uniform over the
// workgroup, no barrier left unmatched.
template <int BLK, int MODE, bool TIES, bool RUNS = false> __global__ void __launch_bounds__(NT) kTrellis(const DevTables *__restrict__ T, const BatchView *__restrict__ B) {
    static_assert(!RUNS || MODE == 0, "runs are pass 1");
    __shared__ TrellisLds lds;
    int sg = blockIdx.x, sgEnd = sg + 1;
    if constexpr (RUNS) { // (scalar: the loop below is the workgroup's, not the lane's)
        sg = __builtin_amdgcn_readfirstlane(B->runSeg0[blockIdx.x]);
        sgEnd = __builtin_amdgcn_readfirstlane(B->runSeg0[blockIdx.x + 1]);
    }
    for (;;) {
        if constexpr (!TIES) {
            const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
            switch (w) {
                case 0: trellisPiece<BLK, MODE, TIES, 0>(*T, *B, lds, sg); break;
                case 1: trellisPiece<BLK, MODE, TIES, 1>(*T, *B, lds, sg); break;
                case 2: trellisPiece<BLK, MODE, TIES, 2>(*T, *B, lds, sg); break;
                case 3: trellisPiece<BLK, MODE, TIES, 3>(*T, *B, lds, sg); break;
                case 4: trellisPiece<BLK, MODE, TIES, 4>(*T, *B, lds, sg); break;
                case 5: trellisPiece<BLK, MODE, TIES, 5>(*T, *B, lds, sg); break;
                case 6: trellisPiece<BLK, MODE, TIES, 6>(*T, *B, lds, sg); break;
                default: trellisPiece<BLK, MODE, TIES, 7>(*T, *B, lds, sg); break;
            }
        } else
            trellisPiece<BLK, MODE, TIES>(*T, *B, lds, sg);
        if (!RUNS || ++sg >= sgEnd) break; // (uniform: the run's bounds are the workgroup's)
        BLOCK_SYNC();
    }
}

namespace augx { namespace dev {
void AUGX_TU_NAME(launchTrellis_)(int mode, bool ties, unsigned grid, hipStream_t st, const DevTables *T, const BatchView *B) {
    constexpr int BLK = AUGX_TU_BLK;
#define L(MODE_) do { if (ties) hipLaunchKernelGGL((kTrellis<BLK, MODE_, true>), dim3(grid), dim3(NT), 0, st, T, B); \
                      else hipLaunchKernelGGL((kTrellis<BLK, MODE_, false>), dim3(grid), dim3(NT), 0, st, T, B); } while (0)
    if (mode == TRELLIS_RUNS) { // pass 1 in runs: grid = the runs of the plan
        if (ties) hipLaunchKernelGGL((kTrellis<BLK, 0, true, true>), dim3(grid), dim3(NT), 0, st, T, B);
        else hipLaunchKernelGGL((kTrellis<BLK, 0, false, true>), dim3(grid), dim3(NT), 0, st, T, B);
        return;
    }
    switch (mode) { case 0: L(0); break; case 1: L(1); break; case 2: L(2); break; default: L(3); break; }
#undef L
}
}} // namespace
