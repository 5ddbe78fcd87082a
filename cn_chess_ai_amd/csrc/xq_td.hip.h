// xq_td.hip.h — the TD rule of a step, stated once on the device (outputLayerDeltaKernel dqn.cu:288-295 on the one non-zero column of
// chessai.cpp:121-133): the fold of the partial maxima, target, loss objects, output delta, top hidden delta, per-sample record and priority
// write-back, with the TD delta kernels and the TD-error statistics.  td_delta_kernel / td_delta_huber_kernel (xq_td_delta.inc.h), level 3 of
// qmax_refine2_kernel<256, true> and per_writeback_kernel call the helpers.  (included by xq_dqn.hip in front of xq_refine.hip.h)
#pragma once

namespace xq {

// THE first-maximum rule of a fold that carries row indices (Double DQN): v takes over where it is larger, or equal with the smaller row.
__device__ __forceinline__ void first_max_take(float& m, int& mi, const float v, const int vi) { if (v > m || (v == m && vi < mi)) { m = v; mi = vi; } }

// zmax[b] = max over the column-max GEMM's partial rows t of partial[t][b] (and, for Double DQN, the row index that came with
// the first maximum).  The partials are [n_partial][n]: a block takes 64 consecutive samples so that every wave-instruction reads
// 256 contiguous bytes of one partial row (td_delta_kernel's one-wave-per-sample walk touched a cache line per value); wave w
// folds rows w, w+4, ... with 8 independent loads in flight, the four waves combine through LDS.
// blockIdx.y = one of kReduceParts contiguous ranges of partial rows (4x the blocks in flight: the kernel is pure latency);
// zmax / zidx are [kReduceParts][n], td_delta_kernel folds the last kReduceParts values of its sample itself.
enum { kReduceParts = 4 };
__global__ __launch_bounds__(256) void colmax_reduce_kernel(const float* __restrict__ partial_all, const int* __restrict__ partial_idx_all,
                                                            int n_partial_all, int n, long long ld, float* __restrict__ zmax_all,
                                                            int* __restrict__ zidx_all) {
    const int per = (n_partial_all + kReduceParts - 1) / kReduceParts;
    const int t0 = (int)blockIdx.y * per;
    const int n_partial = max(0, min(per, n_partial_all - t0));
    const float* partial = partial_all + (long long)t0 * ld;          // rows of the partial arrays are `ld` apart (>= n)
    const int* partial_idx = partial_idx_all ? partial_idx_all + (long long)t0 * ld : nullptr;
    float* zmax = zmax_all + (long long)blockIdx.y * n;
    int* zidx = zidx_all + (long long)blockIdx.y * n;
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
    const int lane = (int)(threadIdx.x & 63), wid = (int)(threadIdx.x >> 6);
    const int b = (int)blockIdx.x * 64 + lane;
    const bool ok = b < n;
    float m = -__builtin_inff();
    int mi = 0x7fffffff;
    const bool arg = partial_idx != nullptr;
    int t = wid;
    for (; t + 28 < n_partial; t += 32) {
        float v[8];
        int vi[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            v[u] = ok ? partial[(long long)(t + 4 * u) * ld + b] : -__builtin_inff();
            vi[u] = (ok && arg) ? partial_idx[(long long)(t + 4 * u) * ld + b] : 0x7fffffff;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (arg) first_max_take(m, mi, v[u], vi[u]);
            else m = fmaxf(m, v[u]);
        }
    }
    for (; t < n_partial; t += 4) {
        const float v = ok ? partial[(long long)t * ld + b] : -__builtin_inff();
        const int vi = (ok && arg) ? partial_idx[(long long)t * ld + b] : 0x7fffffff;
        if (arg) first_max_take(m, mi, v, vi);
        else m = fmaxf(m, v);
    }
    sv[wid][lane] = m; si[wid][lane] = mi;
    __syncthreads();
    if (wid == 0 && ok) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float v = sv[w][lane];
            const int vi = si[w][lane];
            if (arg) first_max_take(m, mi, v, vi);
            else m = fmaxf(m, v);
        }
        zmax[b] = m;
        if (arg) zidx[b] = mi;
    }
}
// The (up to kReduceParts) maxima left for sample b, without a row index: every load unconditional, rows past n_partial - 1 read the last one again
__device__ __forceinline__ float td_fold_max(const float* __restrict__ partial, const int n, const int b, const int n_partial) {
    float zm = partial[b];
#pragma unroll
    for (int t = 1; t < kReduceParts; ++t) zm = fmaxf(zm, partial[(long long)min(t, n_partial - 1) * n + b]);
    return zm;
}

// What the generalised TD step (BASELINE configs[4], build-defined) adds to td_delta_kernel; all optional.
struct TdExtra {
    const int* partial_idx;        // Double DQN: row index of the maximum of every sample (first maximum), reduced
    const float* wout_t; const uint16_t* wout_t_bf; const float* bout_t;   // target net's output layer (fp32 master / bf16 shadow)
    const float* alast_t; const uint16_t* alast_t_bf;                      // a_last(s') of the target net (fp32 / bf16 bits)
    const uint16_t* wout_bf;       // bf16 Q-net: shadow of the online output layer for Q(s,a)
    const float* is_w; const float* is_wmax;     // prioritized replay: raw importance weights [n] and their batch maximum
    float* prio; unsigned* pmax_live;            // prioritized replay: priority table (by ring slot) and the running maximum (float bits)
    float per_eps, per_alpha;
    int double_dqn, nout;
    uint16_t* dtop_bf;             // XQ_PRECISION_BF16_FULL: the top hidden delta rounded to bf16 beside the fp32 one
};

// The TD loss as a step object (DESIGN.md section 4 "TD loss"), stated once for every place that forms the output delta: with
// e = fl32(q - y), err(e) is dL/dq, the factor that stands where (q - y) stood, and loss(e) the sample's entry of lossv.
//   squared:  err = e                       loss = 0.5f e e
//   huber(k): err = min(max(e, -k), k)      loss = |e| <= k ? 0.5f e e : k (|e| - 0.5f k)          (k > 0, +inf allowed)
// Where |e| <= k the clamp returns e itself, so huber(k) with k above every |e| of a batch has the bits of the squared loss.  The
// priority of prioritized replay is taken from the raw error, never from err(e).
// The tanh derivative 1 - q^2 of the output delta, the product rounded on its own: the squared-loss kernels have always formed it so (the
// subtraction shares one packed add with q - y, which leaves no fma to contract), and the fixed point above needs every loss to round alike.
__device__ __forceinline__ float td_dtanh(const float q) {
#pragma clang fp contract(off)
    const float qq = q * q;
    return 1.f - qq;
}
struct SquaredLoss {
    __device__ __forceinline__ float err(const float e) const { return e; }
    __device__ __forceinline__ float loss(const float e) const { return 0.5f * e * e; }
};
struct HuberLoss {
    float kappa;
    __device__ __forceinline__ float err(const float e) const { return fminf(fmaxf(e, -kappa), kappa); }
    __device__ __forceinline__ float loss(const float e) const {
        const float a = fabsf(e);
        return a <= kappa ? 0.5f * e * e : kappa * (a - 0.5f * kappa);
    }
};

// THE rule of a TD step, each piece once.  zm: pre-activation of the bootstrap value (max_k tanh(z_k) = tanh(max_k z_k)); gamma: signed by the host (zero-sum:
// negated); q: the caller's (the refine kernel has it long before zm); isw: w_b / max w of prioritized replay, else 1.f (exact); dtop = 0 without a view row.
__device__ __forceinline__ float td_target(const float r, const bool done, const float gamma, const float zm) { return done ? r : r + gamma * tanhf(zm); }
template <class Loss>
__device__ __forceinline__ float td_output_delta(const Loss& L, const float q, const float y, const float isw) { return L.err(q - y) * td_dtanh(q) * isw; }
__device__ __forceinline__ float td_top_delta(const float delta, const float view, const float act) { return delta * view * (1.f - act * act); }
__device__ __forceinline__ float4 td_top_delta(const bool on, const float delta, const float4 view, const float4 act) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) {
        o.x = td_top_delta(delta, view.x, act.x); o.y = td_top_delta(delta, view.y, act.y);
        o.z = td_top_delta(delta, view.z, act.z); o.w = td_top_delta(delta, view.w, act.w);
    }
    return o;
}
// The per-sample record of a step, by the one lane that holds the sample: a sample that is not live leaves delta 0, action -1, loss 0.
template <class Loss>
__device__ __forceinline__ void td_record_store(const Loss& L, float* __restrict__ dsc, int32_t* __restrict__ act, float* __restrict__ qsa, float* __restrict__ yv,
                                                float* __restrict__ lossv, const int b, const bool live, const int a, const float delta, const float q, const float y) {
    dsc[b] = delta;
    act[b] = live ? a : -1;
    qsa[b] = q; yv[b] = y;
    lossv[b] = live ? L.loss(q - y) : 0.f;
}
// Prioritized replay: prio[slot] = (|q - y| + eps)^alpha, from the raw error.  The running maximum rarely moves once training is under way: test first, so
// that 16 K waves do not queue on one address (positive floats order like their bit patterns; a maximum is order-independent, hence still deterministic).
__device__ __forceinline__ void per_priority_store(float* __restrict__ prio, unsigned* pmax_live, const int slot, const float q, const float y,
                                                   const float eps, const float alpha) {
    const float p = powf(fabsf(q - y) + eps, alpha);
    prio[slot] = p;
    if (__float_as_uint(p) > __hip_atomic_load(pmax_live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(pmax_live, __float_as_uint(p));
}

// TD target, output delta and the TOP hidden delta for one sample per wave (chessai.cpp:122-128 +
// outputLayerDeltaKernel dqn.cu:288-295 + hiddenLayerDeltaKernel dqn.cu:297-308 for the last hidden layer).
// The output delta of a TD step has ONE non-zero entry per sample (column action.to), so the last hidden layer's delta
// is a scaled row of the weight view — no GEMM:  dtop[b][i] = delta_b * View[a_b][i] * (1 - a_last[b][i]^2), where
// View[a][i] = view[a*view_ld + i] is the as-written (reference mode: a < view_kmax = width of the last hidden layer,
// stride = width of the layer below) or the textbook (row a of W_out) operand.  Also emits, per sample, the scalar
// delta and the action (gathered through `slots`) for the segmented output-layer gradient.
// Double DQN: the partials carry (max z_online(s'), its row a*); y = r + gamma * tanh(W_out_target[a*] . a_last_target(s') + b).
// Prioritized replay: delta is scaled by w_b / max w, and (|Q(s,a) - y| + eps)^alpha goes back into the priority table.
// td_delta_kernel (squared loss; name, arguments and instructions as ever) and td_delta_huber_kernel (kappa behind the last argument)
#define XQ_TD_DELTA_KERNEL td_delta_kernel
#define XQ_TD_DELTA_LOSS_PARAM
#define XQ_TD_DELTA_LOSS const SquaredLoss L{}
#include "xq_td_delta.inc.h"
#undef XQ_TD_DELTA_KERNEL
#undef XQ_TD_DELTA_LOSS_PARAM
#undef XQ_TD_DELTA_LOSS
#define XQ_TD_DELTA_KERNEL td_delta_huber_kernel
#define XQ_TD_DELTA_LOSS_PARAM , float kappa
#define XQ_TD_DELTA_LOSS const HuberLoss L{kappa}
#include "xq_td_delta.inc.h"
#undef XQ_TD_DELTA_KERNEL
#undef XQ_TD_DELTA_LOSS_PARAM
#undef XQ_TD_DELTA_LOSS

// TD-error summary of the last step (xq_dqn_td_error_stats; on request only, never part of a step): over the live samples of qsa / yv /
// act, with e = fl32(q - y) as the step formed it: their number, sum |e| and sum loss in fp64 (the loss of e evaluated in fp64: squared
// = huber(+inf)), max |e| and the number with |e| > kappa.  ONE block of 256 threads: thread t takes samples t, t + 256, .. in ascending
// order, contraction off; then grad_norm_kernel's tree — __shfl_down by 32, 16, .. 1 in each wave, ((w0 + w1) + w2) + w3 — so the record
// does not depend on the device.  Thread 0 writes it with plain stores.
struct TdStatsRecord {         // 48 bytes
    unsigned long long live;
    double sum_abs, sum_loss, max_abs;
    unsigned long long linear, samples;
};
__device__ __forceinline__ void td_stats_add(const double kd, const float e, double& sa, double& sl) {
#pragma clang fp contract(off)
    const double a = (double)fabsf(e);
    const double h = 0.5 * a;
    const double hk = 0.5 * kd;
    const double d = a - hk;
    sa = sa + a;
    sl = sl + (a <= kd ? h * a : kd * d);
}
__global__ __launch_bounds__(256) void td_error_stats_kernel(const float* __restrict__ qsa, const float* __restrict__ yv,
                                                             const int32_t* __restrict__ act, int n, float kappa, TdStatsRecord* __restrict__ rec) {
    const int tid = (int)threadIdx.x;
    const double kd = (double)kappa;
    unsigned long long live = 0, lin = 0;
    double sa = 0.0, sl = 0.0;
    float mx = 0.f;
    for (int b = tid; b < n; b += 256) {
        if (act[b] < 0) continue;                      // td_delta_kernel left -1 for a sample that is not live
        const float e = qsa[b] - yv[b];
        td_stats_add(kd, e, sa, sl);
        mx = fmaxf(mx, fabsf(e));
        live += 1;
        if (fabsf(e) > kappa) lin += 1;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        sa += __shfl_down(sa, off, 64);
        sl += __shfl_down(sl, off, 64);
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
        live += __shfl_down(live, off, 64);
        lin += __shfl_down(lin, off, 64);
    }
    __shared__ double wsa[4], wsl[4];
    __shared__ float wmx[4];
    __shared__ unsigned long long wlive[4], wlin[4];
    if ((tid & 63) == 0) { const int w = tid >> 6; wsa[w] = sa; wsl[w] = sl; wmx[w] = mx; wlive[w] = live; wlin[w] = lin; }
    __syncthreads();
    if (tid == 0) {
        rec->live = ((wlive[0] + wlive[1]) + wlive[2]) + wlive[3];
        rec->sum_abs = ((wsa[0] + wsa[1]) + wsa[2]) + wsa[3];
        rec->sum_loss = ((wsl[0] + wsl[1]) + wsl[2]) + wsl[3];
        rec->max_abs = (double)fmaxf(fmaxf(fmaxf(wmx[0], wmx[1]), wmx[2]), wmx[3]);
        rec->linear = ((wlin[0] + wlin[1]) + wlin[2]) + wlin[3];
        rec->samples = (unsigned long long)n;
    }
}

}  // namespace xq
