// Average precision, ROC-AUC and MRR of one validation batch, computed where ops.edge_score
// left the scores: what the reference's evaluate() gets from scikit-learn after
// torch.cat([pred_pos, pred_neg]).sigmoid().cpu() (scripts/offline_edge_prediction.py:141-146).
//
// Nothing is sorted.  With pos[P] and neg[N], every metric is a sum over the positives of
// integer counts, the float32 values compared as IEEE compares them (-0 == +0), so ties come
// out right by construction:
//
//   pge_i = #{j : pos[j] >= pos[i]}      nge_i = #{k : neg[k] >= pos[i]}
//   nlt_i = #{k : neg[k] <  pos[i]}      neq_i = #{k : neg[k] == pos[i]}
//   AP  = (1/P) sum_i pge_i / (pge_i + nge_i)
//   AUC = (sum_i (2 nlt_i + neq_i)) / (2 P N)
//   MRR = (1/P) sum_i 1 / (1 + gt_i + eq_i / 2)        only when N = r P: gt_i / eq_i count
//         positive i's own negatives neg[k P + i], k < r, that are > / == pos[i]
//
// First launch.  One thread owns one positive, 256 to a workgroup.  The workgroup streams the
// P + N scores (pos, then neg) through one LDS tile of kTile floats; every lane reads the same
// LDS word (a broadcast) and keeps pge, nge and ngt = #{neg > pos_i} in registers, from which
// neq = nge - ngt and nlt = N - nge.  Its own r negatives it reads straight from global memory:
// lanes are consecutive in i, so those loads coalesce.  Counts are integers; the quotients and
// their sums are float64 with a correctly rounded division; 2 nlt + neq is summed as uint64.
// The workgroup reduces in a fixed order (lanes by a shuffle tree, then the four waves in
// ascending order) and writes one partial row {sum AP terms, sum MRR terms, AUC numerator,
// non-finite flag}.  Every workgroup sees every score, so every row carries the same flag.
//
// Second launch (as edge_score.hip finishes its partial rows): one workgroup stages the at most
// kLinkMetricsMaxPartialRows rows in LDS and thread 0 sums them in index order, divides, writes
// out[3] and updates the accumulator with plain loads and stores.  No atomics anywhere: the same
// inputs give the same bits.  A NaN or an infinity among the scores turns the three outputs into
// NaN and adds 1 to the accumulator's nonfinite field, nothing else: the host never has to wait
// to learn about it.
#include "block_ops.hpp"
#include "common.hpp"

#include <cmath>
#include <cstdint>

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kTile = static_cast<uint32_t>(kLinkMetricsTile);
static_assert(kTile % kThreads == 0, "a tile is loaded in whole passes of the workgroup");
static_assert(kLinkMetricsMaxPartialRows * kThreads >= kLinkMetricsMaxScores,
              "one partial row per 256 positives");

struct PartialRow {
  double ap;          // sum of pge / (pge + nge) over the workgroup's positives
  double mrr;         // sum of 1 / (1 + gt + eq / 2); 0 without MRR
  uint64_t auc;       // sum of 2 nlt + neq
  uint64_t nonfinite; // 1 when a score is NaN or infinite
};
static_assert(sizeof(PartialRow) == kLinkMetricsPartialWords * 8, "row layout");

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_down(v, off, kWave);
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1)
    v += static_cast<uint64_t>(__shfl_down(static_cast<unsigned long long>(v), off, kWave));
  return v;
}

__global__ void __launch_bounds__(kThreads)
link_metrics_count(const float* __restrict__ pos, const float* __restrict__ neg, uint32_t P,
                   uint32_t N, uint32_t r, PartialRow* __restrict__ partials) {
  __shared__ float tile[kTile];
  __shared__ double s_ap[kWaves], s_mrr[kWaves];
  __shared__ uint64_t s_auc[kWaves];
  __shared__ int s_bad[kWaves];
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;
  const bool own = i < P;
  const float x = own ? pos[i] : 0.f;
  const uint32_t total = P + N;      // <= 65536
  uint32_t pge = 0, nge = 0, ngt = 0;
  bool bad = false;
  for (uint32_t g0 = 0; g0 < total; g0 += kTile) {      // uniform over the workgroup
    const uint32_t len = total - g0 < kTile ? total - g0 : kTile;
    for (uint32_t j = threadIdx.x; j < len; j += kThreads) {
      const uint32_t g = g0 + j;      // < P + N
      const float v = g < P ? pos[g] : neg[g - P];
      bad |= !isfinite(v);
      tile[j] = v;
    }
    __syncthreads();
    const uint32_t np = g0 >= P ? 0u : (P - g0 < len ? P - g0 : len);      // positives first
#pragma unroll 8
    for (uint32_t j = 0; j < np; ++j) pge += tile[j] >= x ? 1u : 0u;
#pragma unroll 8
    for (uint32_t j = np; j < len; ++j) {
      const float v = tile[j];
      nge += v >= x ? 1u : 0u;
      ngt += v > x ? 1u : 0u;
    }
    __syncthreads();
  }
  double q_ap = 0.0, q_mrr = 0.0;
  uint64_t a = 0;
  if (own) {
    const uint32_t neq = nge - ngt, nlt = N - nge;      // finite scores: no unordered compare
    q_ap = static_cast<double>(pge) / static_cast<double>(pge + nge);      // pge >= 1
    a = 2ull * nlt + neq;
    if (r) {
      uint32_t gt = 0, eq = 0;
      for (uint32_t k = 0; k < r; ++k) {
        const float v = neg[static_cast<uint64_t>(k) * P + i];      // k * P + i < r * P = N
        gt += v > x ? 1u : 0u;
        eq += v == x ? 1u : 0u;
      }
      // 1 / (1 + gt + eq / 2), the denominator doubled so that it is an integer
      q_mrr = 2.0 / static_cast<double>(2ull + 2ull * gt + eq);
    }
  }
  // lanes, then waves
  q_ap = wave_sum(q_ap);
  q_mrr = wave_sum(q_mrr);
  a = wave_sum(a);
  const int any_bad = __any(bad ? 1 : 0);
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  if (lane == 0) {
    s_ap[wave] = q_ap;
    s_mrr[wave] = q_mrr;
    s_auc[wave] = a;
    s_bad[wave] = any_bad;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  PartialRow row = {s_ap[0], s_mrr[0], s_auc[0], s_bad[0] ? 1ull : 0ull};
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    row.ap += s_ap[w];
    row.mrr += s_mrr[w];
    row.auc += s_auc[w];
    row.nonfinite |= s_bad[w] ? 1ull : 0ull;
  }
  partials[blockIdx.x] = row;
}

// acc: {sum_ap, sum_auc, sum_mrr, batches, mrr_batches, nonfinite, reserved, reserved}
__global__ void __launch_bounds__(kThreads)
link_metrics_finish(const PartialRow* __restrict__ partials, uint32_t rows, uint32_t P, uint32_t N,
                    uint32_t r, double* __restrict__ out, double* __restrict__ acc) {
  __shared__ PartialRow s[kLinkMetricsMaxPartialRows];
  for (uint32_t p = threadIdx.x; p < rows; p += kThreads) s[p] = partials[p];      // rows <= 256
  __syncthreads();
  if (threadIdx.x != 0) return;
  PartialRow t = s[0];
  for (uint32_t p = 1; p < rows; ++p) {
    t.ap += s[p].ap;
    t.mrr += s[p].mrr;
    t.auc += s[p].auc;
    t.nonfinite |= s[p].nonfinite;
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (t.nonfinite) {
    out[0] = out[1] = out[2] = nan;
    if (acc) acc[5] = acc[5] + 1.0;
    return;
  }
  const double ap = t.ap / static_cast<double>(P);
  // the numerator is an integer below 2^53 and 2 P N <= 2^31: one rounding, in the division
  const double auc = static_cast<double>(t.auc) / (2.0 * static_cast<double>(P) * static_cast<double>(N));
  const double mrr = r ? t.mrr / static_cast<double>(P) : nan;
  out[0] = ap;
  out[1] = auc;
  out[2] = mrr;
  if (!acc) return;
  acc[0] = acc[0] + ap;
  acc[1] = acc[1] + auc;
  acc[3] = acc[3] + 1.0;
  if (r) {
    acc[2] = acc[2] + mrr;
    acc[4] = acc[4] + 1.0;
  }
}

size_t partial_rows(size_t num_pos) { return (num_pos + kThreads - 1) / kThreads; }

}  // namespace

size_t link_metrics_partial_rows(size_t num_pos) {
  GF_REQUIRE(num_pos <= kLinkMetricsMaxScores,
             "link_metrics: more than " + std::to_string(kLinkMetricsMaxScores) + " scores");
  return partial_rows(num_pos);
}

void link_metrics(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                  void* d_partials, size_t partial_rows_given, double* d_out, double* d_acc,
                  int device, hipStream_t stream) {
  GF_REQUIRE(num_pos >= 1 && num_neg >= 1,
             "link_metrics: needs at least one positive and one negative score");
  GF_REQUIRE(num_pos <= kLinkMetricsMaxScores && num_neg <= kLinkMetricsMaxScores &&
                 num_pos + num_neg <= kLinkMetricsMaxScores,
             "link_metrics: more than " + std::to_string(kLinkMetricsMaxScores) + " scores");
  GF_REQUIRE(d_pos && d_neg && d_out, "link_metrics: null pos, neg or out");
  const size_t rows = partial_rows(num_pos);
  GF_REQUIRE(d_partials != nullptr && partial_rows_given >= rows,
             "link_metrics: partials buffer missing or smaller than "
             "gf_link_metrics_partial_rows() asks for");
  const uint32_t P = static_cast<uint32_t>(num_pos), N = static_cast<uint32_t>(num_neg);
  const uint32_t r = N % P == 0 ? N / P : 0;      // 0: no MRR
  PartialRow* partials = static_cast<PartialRow*>(d_partials);
  DeviceGuard dg(device);
  link_metrics_count<<<dim3(static_cast<uint32_t>(rows)), dim3(kThreads), 0, stream>>>(
      d_pos, d_neg, P, N, r, partials);
  GF_HIP(hipGetLastError());
  link_metrics_finish<<<dim3(1), dim3(kThreads), 0, stream>>>(
      partials, static_cast<uint32_t>(rows), P, N, r, d_out, d_acc);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
