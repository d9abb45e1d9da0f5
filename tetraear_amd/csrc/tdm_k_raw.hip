// libtetrahip.so, raw-integer decimator translation unit: k_pz_raw per decimation factor, compiled in two
// halves (-DTDM_RAW_PART=0 / 1) (gfx950 only).
#include <cstdio>

#include "dev_comm.hpp"
#include "launch.hpp"

namespace tdm {

// raw-integer decimator (pz_raw_body), one launch for all blocks of all rows: blocks without extension samples run the
// narrow body (bytes as they come), the first block and the block(s) with the tail extension the wide one (int16 pairs)
// FOLD: the narrow blocks in the folded block-sum form (pz_raw_fold_lane) where one exists for Q; the per-sample form is
// kept as a second instantiation for those Q only (tdm_debug_set "raw_fold" 0: the A/B partner)
// PRUNE: the lane scans without the terms PzScanKeep<Q, S> leaves out; every factor whose table leaves any out keeps the
// form with every term as a second instantiation (tdm_debug_set "scan_prune" 0; a design the table does not fit)
template <int Q, int S>
struct PzRawPrunes {
    static constexpr bool value = PzScanKeep<Q, S>::kept(0) + PzScanKeep<Q, S>::kept(1) + PzScanKeep<Q, S>::kept(2) + PzScanKeep<Q, S>::kept(3) < 4 * kPzScanTerms;
};

template <int Q, int S, int EDGE, int FMT8, bool FOLD, bool PRUNE>
__global__ __launch_bounds__(64, 2) void k_pz_raw(const ZpParams P, const void *iq, int64_t stride, int b_tail)
{
    __shared__ __attribute__((aligned(16))) double stg[PzRawScratch<Q, S, EDGE, FOLD>::kDoubles];
    WaveComm cm{stg};
    const int blk = (int)blockIdx.x;
    if (blk == 0 || blk >= b_tail)
        pz_raw_body<Q, S, EDGE, FMT8, true, true, PRUNE>(P, iq, stride, cm, (int)threadIdx.x, blk, (int)blockIdx.y);
    else
        pz_raw_body<Q, S, EDGE, FMT8, false, FOLD, PRUNE>(P, iq, stride, cm, (int)threadIdx.x, blk, (int)blockIdx.y);
}

template <int Q, int S, int EDGE, int FMT8, bool PRUNE>
static void launch_pz_raw_form(const ZpParams &P, const void *iq, int64_t stride, int b_tail, int rows, bool fold, hipStream_t st)
{
    if (PzRawFold<Q>::value && !fold)
        hipLaunchKernelGGL((k_pz_raw<Q, S, EDGE, FMT8, false, PRUNE>), dim3(P.nb, rows), dim3(64), 0, st, P, iq, stride, b_tail);
    else
        hipLaunchKernelGGL((k_pz_raw<Q, S, EDGE, FMT8, PzRawFold<Q>::value, PRUNE>), dim3(P.nb, rows), dim3(64), 0, st, P, iq, stride, b_tail);
}

template <int Q, int S, int EDGE, int FMT8>
void launch_pz_raw(const ZpParams &P, const void *iq, int64_t stride, int b_tail, int rows, bool fold, bool prune, hipStream_t st)
{
    if (PzRawPrunes<Q, S>::value && !prune)
        launch_pz_raw_form<Q, S, EDGE, FMT8, false>(P, iq, stride, b_tail, rows, fold, st);
    else
        launch_pz_raw_form<Q, S, EDGE, FMT8, PzRawPrunes<Q, S>::value>(P, iq, stride, b_tail, rows, fold, st);
}

#define TDM_PZR_INST(Q, S) template void launch_pz_raw<Q, S, kEdgeSos, FMT_CU8>(const ZpParams &, const void *, int64_t, int, int, bool, bool, hipStream_t);
#if TDM_RAW_PART == 0
TDM_PZR_CASES_A(TDM_PZR_INST)
#else
TDM_PZR_CASES_B(TDM_PZR_INST)
#endif
#undef TDM_PZR_INST

}  // namespace tdm
