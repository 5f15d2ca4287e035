// iq_search.hpp -- the ONE grid search of the I/Q calibration (include/iqgpu.h: iqgpu_iq_optimizer_calibrate with the host metric,
// iqgpu_chain_calibrate_iq with k_iq_metric) and the constants both evaluators share.  Plain C++: the optimiser includes nothing of HIP.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/iqgpu.h"

namespace iqgpu {

constexpr int kIqN = 1024;               // IQ_CORRECTION_FFT_SIZE: samples of a block, points of the transform
constexpr int kIqBinLo = 25, kIqBinHi = 486;   // (int)(0.05f * 512), (int)(0.95f * 512): the bins i of the utility (iq_correct.c:339-360)
constexpr int kIqCandTile = 16;          // candidates per wave of k_iq_metric
constexpr int kIqCandsPerLaunch = 256;   // candidates per launch of k_iq_metric (a whole 15 x 15 grid); longer lists: several launches

// ---- the search (iq_optimizer.cpp) ----
// The evaluator fills metric[b * n_cand + c] for every block b < n_blocks and every candidate, and -- where power_range_db is not
// NULL: the first call of a search -- power_range_db[b] (_estimate_power of block b, iq_correct.c:362-389).  Returns an IQGPU_ code.
typedef int (*IqCalibEval)(void *user, const iqgpu_iq_cand *cands, size_t n_cand, float *metric, float *power_range_db);
// IQGPU_OK, or IQGPU_EINVAL with *why naming the option (o may be NULL)
int iq_calib_check_opts(const iqgpu_iq_calib_opts *o, const char **why);
// the levels of include/iqgpu.h over n_blocks blocks; o has passed iq_calib_check_opts; *rep is filled (blocks_taken = n_blocks)
int iq_calib_search(const iqgpu_iq_calib_opts &o, size_t n_blocks, IqCalibEval eval, void *user, iqgpu_iq_calib_report *rep);

} // namespace iqgpu

