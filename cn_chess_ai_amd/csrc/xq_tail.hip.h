// xq_tail.hip.h — the gradient half of a TD step: partial-maximum fold, TD target / output delta (outputLayerDeltaKernel dqn.cu:288-295 on
// the one non-zero column of chessai.cpp:121-133), output-layer and bias gradients as ordered sums, the fused launches (td_tail_kernel), the
// ordered slab reduction, the Q head finish and the SGD step (updateWeightsBiasesKernel dqn.cu:310-319, batched)
// (kernel half of xq_dqn.hip, split out in round 5; included by xq_dqn.hip only, inside namespace xq)
#pragma once

namespace xq {

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
            if (arg) { if (v[u] > m || (v[u] == m && vi[u] < mi)) { m = v[u]; mi = vi[u]; } }
            else m = fmaxf(m, v[u]);
        }
    }
    for (; t < n_partial; t += 4) {
        const float v = ok ? partial[(long long)t * ld + b] : -__builtin_inff();
        const int vi = (ok && arg) ? partial_idx[(long long)t * ld + b] : 0x7fffffff;
        if (arg) { if (v > m || (v == m && vi < mi)) { m = v; mi = vi; } }
        else m = fmaxf(m, v);
    }
    sv[wid][lane] = m; si[wid][lane] = mi;
    __syncthreads();
    if (wid == 0 && ok) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float v = sv[w][lane];
            const int vi = si[w][lane];
            if (arg) { if (v > m || (v == m && vi < mi)) { m = v; mi = vi; } }
            else m = fmaxf(m, v);
        }
        zmax[b] = m;
        if (arg) zidx[b] = mi;
    }
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

// Output-layer gradient of a TD minibatch: gW_out[j][:] = sum over the samples with action.to == j of delta_b * a_last[b][:]
// and gb_out[j] = sum of delta_b (j < 96).  Segmented sums instead of a [96 x B] x [B x H] product: every sample's
// activation row is read exactly once.  Block (group of 4 actions, chunk of samples): ordered compaction of the chunk's
// samples whose action falls in the group, then the rows are streamed into per-wave LDS accumulators (combined in fixed
// order => bitwise reproducible).  partial[chunk][96*H + 96] (weights, then biases).
__device__ __forceinline__ void out_grad_block(const int32_t* __restrict__ act, const float* __restrict__ dsc,
                                               const float* __restrict__ a_last, int n, int H, int chunk,
                                               float* __restrict__ partial, int g /* actions 4g .. 4g+3 */, int chunk_id, float* __restrict__ smem) {
    float* acc = smem;                                  // [4 waves][4 actions][H]
    uint16_t* list = reinterpret_cast<uint16_t*>(smem + 16 * H);   // [chunk] (b_local | class << 11)
    __shared__ int total;
    __shared__ float bsum[4][4];
    const int c0 = chunk_id * chunk, c1 = min(n, c0 + chunk);
    const int tid = (int)threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // the chunk's actions first (all loads of a thread in flight together), accumulator zeroing under their latency; then the
    // ordered compaction with two barriers in all: per-wave counts of every round published first, offsets = prefix sums over
    // (round, wave) that every thread computes for itself
    constexpr int kMaxIters = 8;                         // chunk <= 2048
    __shared__ int wc[kMaxIters][4];
    int clsv[kMaxIters];
#pragma unroll
    for (int it = 0; it < kMaxIters; ++it) {
        const int b = c0 + it * 256 + tid;
        const int a = act[min(b, c1 - 1)];                // unconditional, clamped (see l0_grad_kernel)
        clsv[it] = (b < c1 && a >= 4 * g && a < 4 * g + 4) ? a - 4 * g : -1;
    }
    for (int i = tid; i < 16 * H; i += 256) acc[i] = 0.f;
#pragma unroll
    for (int it = 0; it < kMaxIters; ++it) {
        const unsigned long long m = __ballot(clsv[it] >= 0);
        if (lane == 0) wc[it][wid] = __popcll(m);
    }
    __syncthreads();
    {
        const int iters = (c1 - c0 + 255) / 256;
        int off = 0;
#pragma unroll
        for (int it = 0; it < kMaxIters; ++it) {
            if (it < iters) {
                const unsigned long long m = __ballot(clsv[it] >= 0);
                int o = off;
                for (int w = 0; w < wid; ++w) o += wc[it][w];
                if (clsv[it] >= 0) list[o + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)((it * 256 + tid) | (clsv[it] << 11));
            }
            off += wc[it][0] + wc[it][1] + wc[it][2] + wc[it][3];
        }
        if (tid == 0) total = off;
    }
    __syncthreads();
    const int cnt = total;
    float* my = acc + (long long)wid * 4 * H;
    float bs0 = 0.f, bs1 = 0.f, bs2 = 0.f, bs3 = 0.f;
    // wave w takes entries w, w+4, ... (fixed assignment), 8 rows in flight
    int i = wid;
    for (; i + 28 < cnt; i += 32) {
        int bb[8], cl[8];
        float dl[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = list[i + 4 * u];
            bb[u] = c0 + (e & 2047); cl[u] = e >> 11;
            dl[u] = dsc[bb[u]];
        }
        for (int col = lane * 4; col < H; col += 256) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 x = *reinterpret_cast<const float4*>(a_last + (long long)bb[u] * H + col);
                v[u].x = x.x; v[u].y = x.y; v[u].z = x.z; v[u].w = x.w;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float4* a = reinterpret_cast<float4*>(my + cl[u] * H + col);
                float4 t = *a;
                t.x += dl[u] * v[u].x; t.y += dl[u] * v[u].y; t.z += dl[u] * v[u].z; t.w += dl[u] * v[u].w;
                *a = t;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (cl[u] == 0) bs0 += dl[u]; else if (cl[u] == 1) bs1 += dl[u]; else if (cl[u] == 2) bs2 += dl[u]; else bs3 += dl[u];
        }
    }
    for (; i < cnt; i += 4) {
        const int e = list[i];
        const int b = c0 + (e & 2047), cls = e >> 11;
        const float d1 = dsc[b];
        if (cls == 0) bs0 += d1; else if (cls == 1) bs1 += d1; else if (cls == 2) bs2 += d1; else bs3 += d1;
        for (int col = lane * 4; col < H; col += 256) {
            const float4 x = *reinterpret_cast<const float4*>(a_last + (long long)b * H + col);
            float4* a = reinterpret_cast<float4*>(my + cls * H + col);
            float4 t = *a;
            t.x += d1 * x.x; t.y += d1 * x.y; t.z += d1 * x.z; t.w += d1 * x.w;
            *a = t;
        }
    }
    if (lane == 0) { bsum[wid][0] = bs0; bsum[wid][1] = bs1; bsum[wid][2] = bs2; bsum[wid][3] = bs3; }
    __syncthreads();
    float* out = partial + (long long)chunk_id * (96LL * H + 96);
    for (int i = tid; i < 4 * H; i += 256)
        out[(long long)4 * g * H + i] = ((acc[i] + acc[4 * H + i]) + acc[8 * H + i]) + acc[12 * H + i];
    if (tid < 4) out[96LL * H + 4 * g + tid] = ((bsum[0][tid] + bsum[1][tid]) + bsum[2][tid]) + bsum[3][tid];
}
__global__ __launch_bounds__(256) void out_grad_kernel(const int32_t* __restrict__ act, const float* __restrict__ dsc,
                                                       const float* __restrict__ a_last, int n, int H, int chunk,
                                                       float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    out_grad_block(act, dsc, a_last, n, H, chunk, partial, (int)blockIdx.x, (int)blockIdx.y, smem);
}

// dense output delta (general DQN::backpropagate target): d = (q - t) * (1 - q^2)
__global__ void out_delta_dense_kernel(const float* __restrict__ q, const float* __restrict__ t, long long total, float* __restrict__ d) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float a = q[i];
        d[i] = (a - t[i]) * (1.f - a * a);
    }
}

// Bias gradients = column sums of the delta matrices.  All layers of one TD step go through ONE launch (job table)
// of partial sums over row chunks, then ONE ordered reduction launch (deterministic, no atomics).
struct ColsumJobs {
    const float* X[XQ_MAX_LAYERS + 1];
    long long ld[XQ_MAX_LAYERS + 1];
    int C[XQ_MAX_LAYERS + 1];
    float* dst[XQ_MAX_LAYERS + 1];
    long long poff[XQ_MAX_LAYERS + 1];   // first column of the job in the workspace
    int njobs, n, rows_per, R;
    float* work;                         // [R][wld]: row y = the sums over row chunk y, the jobs side by side — for the TD step in the
    long long wld;                       // order of the hidden biases, so that the SGD kernel can take the R rows as slabs (fused_apply)
};
__device__ __forceinline__ void colsum_partial_block(const ColsumJobs& J, int bx, int by, int job) {
    __shared__ float red[4][64];
    const int C = J.C[job];
    const int tx = (int)(threadIdx.x & 63), ty = (int)(threadIdx.x >> 6);
    const int c = bx * 64 + tx;
    if (bx * 64 >= C) return;
    const float* X = J.X[job];
    const long long ld = J.ld[job];
    const int r0 = by * J.rows_per, r1 = min(J.n, r0 + J.rows_per);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < C) {
        int r = r0 + ty;
        for (; r + 12 < r1; r += 16) {
            s0 += X[(long long)r * ld + c];
            s1 += X[(long long)(r + 4) * ld + c];
            s2 += X[(long long)(r + 8) * ld + c];
            s3 += X[(long long)(r + 12) * ld + c];
        }
        for (; r < r1; r += 4) s0 += X[(long long)r * ld + c];
    }
    red[ty][tx] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (ty == 0 && c < C)
        J.work[J.poff[job] + (long long)by * J.wld + c] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}
__global__ __launch_bounds__(256) void colsum_partial_kernel(ColsumJobs J) {
    colsum_partial_block(J, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}
__global__ __launch_bounds__(256) void colsum_final_kernel(ColsumJobs J) {   // 64 columns x 4 partial lanes per block
    __shared__ float red[4][64];
    const int job = (int)blockIdx.y;
    const int C = J.C[job];
    const int tx = (int)(threadIdx.x & 63), ty = (int)(threadIdx.x >> 6);
    const int c = (int)blockIdx.x * 64 + tx;
    if ((int)blockIdx.x * 64 >= C) return;
    // the order of reduce_slabs_kernel / sgd_segments_kernel (four chains z = j, j + 4, ..; ((s0 + s1) + (s2 + s3))): the SGD kernel may
    // sum the rows itself (fused_apply) with the same bits
    float s0 = 0.f;
    if (c < C) {
        const float* p = J.work + J.poff[job] + c;
        const int R4 = J.R & ~3;
        for (int z = ty; z < R4; z += 4) s0 += p[(long long)z * J.wld];
        if (ty == 0) for (int z = R4; z < J.R; ++z) s0 += p[(long long)z * J.wld];     // the leftover rows continue chain 0, as there
    }
    red[ty][tx] = s0;
    __syncthreads();
    if (ty == 0 && c < C) J.dst[job][c] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}

// The tail of a TD step as TWO launches on one stream instead of seven on two: every event record on the critical stream costs
// ~6 us of idle time and the join at the end 3-12 us, more than the kernels between them are worth.  One launch
// carries the blocks of several kernels ("horizontal fusion"): the grid is the concatenation of their grids, a block finds its body
// from its linear id (block-uniform branch), dynamic LDS = the largest of the bodies present.  Launch 1 (behind td_delta_kernel,
// once per hidden layer below the top one): the delta GEMM of the next layer down + what only needs the deltas already there — the
// weight-gradient GEMM of the layer above it and, first time round, the output-layer segmented sum.  Launch 2: the layer-0
// segmented sum + the bias column sums.  Long blocks come first in the grid.  Every body is the block function of the stand-alone
// kernel, so the results are bitwise those of the two-stream path (tests/test_dqn_gpu.py).
enum { TAIL_DELTA = 1, TAIL_GRAD = 2, TAIL_OUT = 4, TAIL_COLSUM = 8, TAIL_L0 = 16, TAIL_SEL = 32 };
struct TailArgs {
    // grid order: [l0][grad][delta][out][colsum][sel]; n_* = blocks of each part (0 = absent)
    int n_l0, n_grad, n_delta, n_out, n_colsum, n_sel;
    GemmArgs grad;  int grad_gx, grad_gy;          // 64x64 tiles: grid (gx, gy, splits)
    GemmArgs delta; int delta_gx;                  // grid (gx, gy, 1)
    const int32_t* og_act; const float* og_dsc; const float* og_alast; int og_n, og_H, og_chunk; float* og_partial;   // grid (24, chunks)
    const uint32_t* l0_boards; const float* l0_delta; int l0_n, l0_H, l0_HS, l0_chunk, l0_nsets, l0_nch; float* l0_partial;   // (90, nch, H / HS)
    const uint16_t* l0_planes; long long l0_plane_stride; int l0_kpad, l0_ncb;      // != nullptr: the matrix-pipe form, grid (4, H / 32, nch)
    const uint16_t* l0_sel;                        // ... and its selector half-words (xq_l0grad.hip.h)
    const uint32_t* sel_boards; int sel_n, sel_kpad; uint16_t* sel_out;             // TAIL_SEL: those half-words being made, 64 samples per block
    ColsumJobs cj; int cj_gx, cj_gy;               // grid (gx, R, njobs)
};
// L0MFMA: the layer-0 blocks are the matrix-pipe form (xq_dqn_set_l0_grad_mode(1)) — an instantiation of its own: that body needs 180
// VGPRs against 136 for the rest, and behind a run-time branch in the default kernel it capped every block of the launch at two waves
// per SIMD.  (Measured, same box, 3 x 3 x 300 steps: 180 / 136 / 106 VGPRs — the last forced with amdgpu_waves_per_eu(4) — 0.1887-0.1899 /
// 0.1896-0.1903 / 0.1885-0.1897 ms per step: the launch is not bound by its occupancy.)
template <unsigned KINDS, bool L0MFMA = false>
__global__ __launch_bounds__(256) void td_tail_kernel(const TailArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tail_smem[];
    int b = (int)blockIdx.x;
    if (KINDS & TAIL_L0) {
        if (b < a.n_l0) {
            if (L0MFMA) {
                // column block = b mod (H / 32): workgroups go to the 8 XCDs round-robin in linear order, so every XCD streams ITS columns'
                // planes (1/8 of the 12.6 MB at H = 256: L2-resident) for all row groups and chunks, instead of every XCD streaming half of
                // all planes (PMC: 125 MB of fabric reads per launch with the row group fastest)
                // ... unless the chunks themselves go round the XCDs (8 | chunks): the CHUNK is then the fastest index, XCD x keeps to the planes
                // AND the selector words of its own chunks (1.6 + 0.4 MB of 12.6 + 3.1), nothing is read by two XCDs — with the column block
                // fastest every XCD read all the selector words (25 MB per launch instead of 3.1)
                int rest = b / a.l0_ncb, cb = b % a.l0_ncb, sqg = rest & 3, ch = rest >> 2;
                if ((a.l0_nch & 7) == 0) { ch = b % a.l0_nch; rest = b / a.l0_nch; cb = rest % a.l0_ncb; sqg = rest / a.l0_ncb; }
                l0_grad_mfma_block<0>(a.l0_sel, a.l0_planes, a.l0_plane_stride, a.l0_kpad, a.l0_H, a.l0_chunk, a.l0_partial, sqg, cb, ch,
                                       reinterpret_cast<unsigned char*>(tail_smem));
                return;
            }
            const int per = kSquares * a.l0_nch;
            l0_grad_block(a.l0_boards, a.l0_delta, a.l0_n, a.l0_H, a.l0_HS, a.l0_chunk, a.l0_nsets, a.l0_partial, b % per, a.l0_nch, b / per, tail_smem);
            return;
        }
        b -= a.n_l0;
    }
    if (KINDS & TAIL_GRAD) {
        if (b < a.n_grad) {
            // the k-slab is the fastest index: workgroups go to the XCDs round-robin in linear order, so an XCD keeps to ITS eighth of the
            // samples (both operands: 2 MB) for all tiles, instead of every XCD pulling every slab of both operands through the fabric
            const int per = a.grad_gx * a.grad_gy, nz = a.n_grad / per, z = b % nz, r = b / nz;
            gemm_f32_block<L_MCONTIG, L_MCONTIG, EPI_STORE, 1, 1>(a.grad, r % a.grad_gx, r / a.grad_gx, z, tail_smem, tail_smem + g_tile_floats(64));
            return;
        }
        b -= a.n_grad;
    }
    if (KINDS & TAIL_DELTA) {
        if (b < a.n_delta) {
            gemm_f32_block<L_KCONTIG, L_MCONTIG, EPI_DELTA, 1, 1>(a.delta, b % a.delta_gx, b / a.delta_gx, 0, tail_smem, tail_smem + g_tile_floats(64));
            return;
        }
        b -= a.n_delta;
    }
    if (KINDS & TAIL_OUT) {
        if (b < a.n_out) {
            out_grad_block(a.og_act, a.og_dsc, a.og_alast, a.og_n, a.og_H, a.og_chunk, a.og_partial, b % 24, b / 24, tail_smem);
            return;
        }
        b -= a.n_out;
    }
    if (KINDS & TAIL_COLSUM) {
        if (b < a.n_colsum) {
            const int per = a.cj_gx * a.cj_gy, r = b % per;
            colsum_partial_block(a.cj, r % a.cj_gx, r / a.cj_gx, b / per);
            return;
        }
        b -= a.n_colsum;
    }
    if (KINDS & TAIL_SEL) {
        if (b < a.n_sel) l0_sel_block(a.sel_boards, a.sel_n, a.sel_kpad, a.sel_out, b, reinterpret_cast<uint32_t*>(tail_smem));
    }
}

// ---- ordered slab sums and the segment walk of the optimizers ------------------------------------------------------------------------
// THE order in which partial-sum slabs are added, stated once: four chains z = j, j + 4, .. (leftover slabs continue chain 0), then
// (s0 + s1) + (s2 + s3).  T = float or float4 (element-wise: a quad has the bits of its four elements summed one by one).  Everything
// that promises "the bits of reduce_slabs_kernel" calls this; colsum_final_kernel above spells the same order across four lanes.
__device__ __forceinline__ float vadd(const float a, const float b) { return a + b; }
__device__ __forceinline__ float4 vadd(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ void vzero(float& a) { a = 0.f; }
__device__ __forceinline__ void vzero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
// WHEN the terms are loaded is a separate matter from the order: a loop that loads four terms, waits and adds is a chain of n / 4 dependent
// round trips (17 for the 64 row chunks of the hidden biases), and in a TD step the terms were written a moment ago by other XCDs, so
// every trip goes out to the Infinity Cache.  OrderedSum therefore takes the terms — p[z * st], 0 <= z < n, n the same in every lane of a
// wave — in batches of B (a multiple of 4): all B loads of a batch go out before the first wait, into a statically indexed register array,
// then the terms are added in THE order.
//   whole(): B live terms, straight-line code.
//   part():  0 < n < B live terms: the loads past term n - 1 read that term again (never past the end) and only live terms are added, behind
//            scalar branches.
// Behind the loads stand a scheduling barrier and an empty asm that every loaded value passes through: without the asm the compiler sinks
// each load into the branch that adds it, without the barrier it schedules the first adds (and their waits) between the loads — dependent
// round trips again either way (profiles/NOTES.md, "Ordered sums: every load in flight").
__device__ __forceinline__ void vpin(float& a) { asm volatile("" : "+v"(a)); }
__device__ __forceinline__ void vpin(float4& a) { asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w)); }
template <typename T>
struct OrderedSum {
    T s0, s1, s2, s3;
    __device__ __forceinline__ OrderedSum() { vzero(s0); vzero(s1); vzero(s2); vzero(s3); }
    template <int B>
    __device__ __forceinline__ void whole(const T* __restrict__ p, const long long st) {
        static_assert(B % 4 == 0, "whole groups of four");
        T v[B];
#pragma unroll
        for (int u = 0; u < B; ++u) v[u] = p[u * st];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) vpin(v[u]);
#pragma unroll
        for (int u = 0; u < B; u += 4) { s0 = vadd(s0, v[u]); s1 = vadd(s1, v[u + 1]); s2 = vadd(s2, v[u + 2]); s3 = vadd(s3, v[u + 3]); }
    }
    template <int B>
    __device__ __forceinline__ void part(const T* __restrict__ p, const long long st, const int n) {
        static_assert(B % 4 == 0, "whole groups of four");
        T v[B];
#pragma unroll
        for (int u = 0; u < B; ++u) v[u] = p[min(u, n - 1) * st];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < B; ++u) vpin(v[u]);
#pragma unroll
        for (int u = 0; u < B; u += 4) {
            if (u + 3 < n) {
                s0 = vadd(s0, v[u]); s1 = vadd(s1, v[u + 1]); s2 = vadd(s2, v[u + 2]); s3 = vadd(s3, v[u + 3]);
            } else if (u < n) {                        // the leftover terms continue chain 0
                s0 = vadd(s0, v[u]);
                if (u + 1 < n) s0 = vadd(s0, v[u + 1]);
                if (u + 2 < n) s0 = vadd(s0, v[u + 2]);
            }
        }
    }
    // any n: whole batches of B (a multiple of 4 terms each, so the next batch starts on chain 0 as the order asks), then the rest
    template <int B>
    __device__ __forceinline__ void run(const T* __restrict__ p, const long long st, int n) {
        for (; n >= B; n -= B, p += B * st) whole<B>(p, st);
        if (n > 0) part<B>(p, st, n);
    }
    __device__ __forceinline__ T total() const { return vadd(vadd(s0, s1), vadd(s2, s3)); }
};
// The slab counts of a TD step at the usual sizes (8, 16, 32) are one whole batch each; every other count goes in batches of 64 single
// floats or 32 quads (64 quads would be 256 VGPRs): whatever the library produces (up to 64 slabs) is in flight at once, 33 .. 64 slabs
// of quads in two batches.
template <typename T>
__device__ __forceinline__ T slab_sum(const T* __restrict__ s, int nslabs, long long st, long long i) {   // st, i in units of T
    constexpr int kBatch = sizeof(T) > sizeof(float) ? 32 : 64;
    const T* p = s + i;
    OrderedSum<T> o;
    if (nslabs == 8) o.template whole<8>(p, st);
    else if (nslabs == 16) o.template whole<16>(p, st);
    else if (kBatch > 32 && nslabs == 32) o.template whole<32>(p, st);
    else o.template run<kBatch>(p, st, nslabs);
    return o.total();
}
// out[i] = sum_z slabs[z*stride + i], z ascending (deterministic)
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ slabs, int nslabs, long long stride, long long len, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (long long)gridDim.x * blockDim.x)
        out[i] = slab_sum(slabs, nslabs, stride, i);
}

struct SegTable {
    float* dst[16];
    const float* src[16];
    long long len[16];
    int nslabs[16];            // > 0: src holds that many partial-sum slabs `stride` apart; they are summed here (slab_sum: bit-identical
    long long stride[16];      //      to reducing first), instead of by a kernel of their own
    uint16_t* dst_bf[16];      // bf16 Q-net: shadow of dst, refreshed with the rounded new value (nullptr: none)
    int nseg;
    int reduce_only;           // dst = the slab sum itself (no step): the gradient buffer a reader or an all-reduce needs, in one launch
    int vec4[16];              // set by seg_grid: every pointer 16-byte aligned, len and stride multiples of 4 — four elements per thread
    long long state_off[16];   // where the segment starts in the gradient-buffer layout (layout_td_grads): Adam's m and v, the norm's sums
};

// Q head with the k range split over blocks (q_head) or folded into the last hidden product (EPI_HEAD): q[m][j] = tanh(b_j + the sum of
// the k-slabs of the product), slabs added four at a time as (s0 + s1) + (s2 + s3), the groups of four in ascending order (nslabs even).
// One thread per output.
__global__ __launch_bounds__(256) void q_head_finish_kernel(const float* __restrict__ slabs, long long slab_stride, int nslabs, int n, int n_out, int lds_,
                                                            const float* __restrict__ bias, float* __restrict__ q, int ldq) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * n_out) return;
    const int m = (int)(i / n_out), j = (int)(i % n_out);
    const float* p = slabs + (long long)m * lds_ + j;
    float s = 0.f;
    for (int z = 0; z < nslabs; z += 4) {
        float t = p[z * slab_stride] + p[(z + 1) * slab_stride];
        if (z + 3 < nslabs) t += p[(z + 2) * slab_stride] + p[(z + 3) * slab_stride];
        s = z == 0 ? t : s + t;
    }
    q[(long long)m * ldq + j] = tanhf(bias[j] + s);
}

// bf16 shadow of a weight range (set_params / load_model / set_precision)
__global__ void f32_to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dst[i] = bf16_bits(src[i]);
}
__device__ __forceinline__ void store_bf16(uint16_t* db, long long i, const float v) { db[i] = bf16_bits(v); }
__device__ __forceinline__ uint32_t pack_bf16x2(const float lo, const float hi) { return (uint32_t)bf16_bits(lo) | ((uint32_t)bf16_bits(hi) << 16); }
__device__ __forceinline__ void store_bf16(uint16_t* db, long long i, const float4 v) {
    reinterpret_cast<uint2*>(db)[i] = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
}

// Soft (Polyak) target update (DESIGN.md section 4 "Soft target update"): t' = fmaf(tau, fl32(p_new - t), t), the difference and the fma
// rounded once each, no contraction left to the compiler.  p_new == t gives d = 0 and t' == t exactly: a parameter whose online and
// target bits agree is a fixed point.  SoftArgs rides beside a SegTable (whose layout stays): per segment the target net's pointer and
// its bf16 shadow (nullptr: none).
struct SoftArgs {
    float* tgt[16];
    uint16_t* tgt_bf[16];
    float tau;
};
__device__ __forceinline__ float soft_elem(const float tau, const float p, const float t) {
#pragma clang fp contract(off)
    const float d = p - t;
    return __builtin_fmaf(tau, d, t);
}
__device__ __forceinline__ float soft_elems(const float tau, const float p, const float t) { return soft_elem(tau, p, t); }
__device__ __forceinline__ float4 soft_elems(const float tau, const float4 p, const float4 t) {
    return make_float4(soft_elem(tau, p.x, t.x), soft_elem(tau, p.y, t.y), soft_elem(tau, p.z, t.z), soft_elem(tau, p.w, t.w));
}

// One walk over a SegTable for every optimizer: grid (blocks, segments), block (x, y) strides over segment y.  Per element (T = float) or
// per quad of consecutive elements (T = float4 where t.vec4 says so: 16-byte loads, a quarter of the instructions for the same bytes)
//   g = the gradient-buffer entry, or slab_sum of the pending slabs;  reduce_only: dst = g, nothing else
//   dst = step.elem(dst, g, m, v) — a quad is four calls of the same scalar update, so the bits do not depend on which loop ran —
//   and the bf16 shadow, where there is one, gets the rounded new value.
//   SOFT: the target net's element moves towards the value just produced (soft_elem; a quad is four calls of it) and its shadow follows.
// A step object supplies elem() and kState; with kState it also carries the two state buffers m and v, walked at t.state_off.
template <class Step>
__device__ __forceinline__ float step_elems(const Step& S, const float w, const float g, float& m, float& v) { return S.elem(w, g, m, v); }
template <class Step>
__device__ __forceinline__ float4 step_elems(const Step& S, const float4 w, const float4 g, float4& m, float4& v) {
    float4 o;
    o.x = S.elem(w.x, g.x, m.x, v.x);
    o.y = S.elem(w.y, g.y, m.y, v.y);
    o.z = S.elem(w.z, g.z, m.z, v.z);
    o.w = S.elem(w.w, g.w, m.w, v.w);
    return o;
}
// GridX: this thread's first index along x and the stride of the grid, taken in the __global__ function itself (blockDim read inside an
// inlined device function compiles to a dependent load in the prologue; read in the kernel it is a kernel argument).  The loop: len and
// st in units of T; "slabs or buffer" is asked inside it, the shape that measured fastest (profiles/NOTES.md, "One segment walk").
struct GridX {
    long long first, stride;
};
#define XQ_GRID_X GridX{(long long)blockIdx.x * blockDim.x + threadIdx.x, (long long)gridDim.x * blockDim.x}
template <typename T, bool SLABS, bool SOFT, class Step>
__device__ __forceinline__ void segment_loop(const GridX x, const Step& S, float* d_, const float* s_, long long len, int nslabs, long long st,
                                             uint16_t* db, float* m_, float* v_, bool reduce_only, float* tg_ = nullptr, uint16_t* tb = nullptr,
                                             const float tau = 0.f) {
    T* d = reinterpret_cast<T*>(d_);
    const T* s = reinterpret_cast<const T*>(s_);
    T* ms = reinterpret_cast<T*>(m_);
    T* vs = reinterpret_cast<T*>(v_);
    T* tg = reinterpret_cast<T*>(tg_);
    const bool slabs = SLABS && nslabs > 0;
    if (slabs && reduce_only) {                   // the parameter is not read
        for (long long i = x.first; i < len; i += x.stride) d[i] = slab_sum(s, nslabs, st, i);
        return;
    }
    for (long long i = x.first; i < len; i += x.stride) {
        // the element's own loads first: in flight together with the slab loads, not one more round trip behind them
        const T w = d[i];
        T m, v, tv;
        if (Step::kState) { m = ms[i]; v = vs[i]; }
        else { vzero(m); vzero(v); }
        if (SOFT) tv = tg[i];
        const T g = slabs ? slab_sum(s, nslabs, st, i) : s[i];
        const T o = step_elems(S, w, g, m, v);
        if (Step::kState) { ms[i] = m; vs[i] = v; }
        d[i] = o;
        if (db) store_bf16(db, i, o);
        if (SOFT) {
            const T tn = soft_elems(tau, o, tv);
            tg[i] = tn;
            if (tb) store_bf16(tb, i, tn);
        }
    }
}
// SLABS = false: the table is known to read the gradient buffer only (behind grad_norm_kernel) and the slab sums are not compiled.
// SOFT: Z names the same segments of the target net (never with reduce_only: the host picks a SOFT kernel for a stepping table only).
template <bool SLABS, bool SOFT = false, class Step>
__device__ __forceinline__ void segment_walk(const GridX x, const SegTable& t, const Step& S, float* m = nullptr, float* v = nullptr,
                                             const SoftArgs* Z = nullptr) {
    const int sgm = (int)blockIdx.y;
    if (sgm >= t.nseg) return;
    float* d = t.dst[sgm];
    const float* s = t.src[sgm];
    const long long len = t.len[sgm];
    uint16_t* db = t.dst_bf[sgm];
    if (Step::kState) { m += t.state_off[sgm]; v += t.state_off[sgm]; }
    const int nslabs = SLABS ? t.nslabs[sgm] : 0;
    const long long st = SLABS ? t.stride[sgm] : 0;
    if (SOFT) {
        float* tg = Z->tgt[sgm];
        uint16_t* tb = Z->tgt_bf[sgm];
        if (t.vec4[sgm]) segment_loop<float4, SLABS, true>(x, S, d, s, len >> 2, nslabs, st >> 2, db, m, v, false, tg, tb, Z->tau);
        else segment_loop<float, SLABS, true>(x, S, d, s, len, nslabs, st, db, m, v, false, tg, tb, Z->tau);
        return;
    }
    if (t.vec4[sgm]) segment_loop<float4, SLABS, false>(x, S, d, s, len >> 2, nslabs, st >> 2, db, m, v, t.reduce_only != 0);
    else segment_loop<float, SLABS, false>(x, S, d, s, len, nslabs, st, db, m, v, t.reduce_only != 0);
}

// SGD: dst -= alpha * src per segment (updateWeightsBiasesKernel dqn.cu:310-319, batched form); the compiler's default contraction
struct SgdStep {
    static constexpr bool kState = false;
    float alpha;
    __device__ __forceinline__ float elem(const float w, const float g, float&, float&) const { return w - alpha * g; }
};
__global__ __launch_bounds__(256) void sgd_segments_kernel(SegTable t, float alpha) { segment_walk<true>(XQ_GRID_X, t, SgdStep{alpha}); }
__global__ __launch_bounds__(256) void sgd_segments_soft_kernel(SegTable t, float alpha, SoftArgs Z) { segment_walk<true, true>(XQ_GRID_X, t, SgdStep{alpha}, nullptr, nullptr, &Z); }

// Adam (torch.optim.Adam's formula, amsgrad off, no weight decay; DESIGN.md section 4 "Optimizer"):
//   g' = gs g;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= a m / (sqrt(v) rbc2 + eps)
// a = lr / (1 - b1^t) and rbc2 = 1 / sqrt(1 - b2^t) are computed on the host in double.  m and v live in two fp32 buffers laid out like
// the compact gradient buffer; a parameter that never receives a gradient keeps m = v = 0 and its step is exactly 0.
struct AdamArgs {
    float* m;  float* v;
    float b1, omb1, b2, omb2, eps, a, rbc2, gs;
};
// One element: every product, sum, square root and quotient written out and rounded once, in this order, with no contraction left to
// the compiler.
__device__ __forceinline__ float adam_elem(const AdamArgs& A, float p, float g, float& m, float& v) {
#pragma clang fp contract(off)
    const float gp = A.gs * g;
    const float mg = A.omb1 * gp;
    m = __builtin_fmaf(A.b1, m, mg);
    const float vg = (A.omb2 * gp) * gp;
    v = __builtin_fmaf(A.b2, v, vg);
    const float den = __builtin_fmaf(__builtin_sqrtf(v), A.rbc2, A.eps);
    const float q = m / den;
    return __builtin_fmaf(-A.a, q, p);
}
struct AdamStep {
    static constexpr bool kState = true;
    AdamArgs A;
    __device__ __forceinline__ float elem(const float w, const float g, float& m, float& v) const { return adam_elem(A, w, g, m, v); }
};
__global__ __launch_bounds__(256) void adam_segments_kernel(SegTable t, AdamArgs A) { segment_walk<true>(XQ_GRID_X, t, AdamStep{A}, A.m, A.v); }
__global__ __launch_bounds__(256) void adam_segments_soft_kernel(SegTable t, AdamArgs A, SoftArgs Z) { segment_walk<true, true>(XQ_GRID_X, t, AdamStep{A}, A.m, A.v, &Z); }

// ---- gradient clipping by the global L2 norm (DESIGN.md section 4 "Gradient clipping") ---------------------------------------------
//   S = sum_i (double)g_i^2;  norm = |grad_scale| sqrt(S);  c = (float)min(1, max_norm / (norm + 1e-6))
// grad_norm_kernel walks the segment table of the apply in front of it: grid (kNormBlocks, segments), both fixed by the net alone.
// Element i of a segment belongs to quad i / 4, quad q to thread q mod (kNormBlocks * 256) of the segment's blocks; a thread adds the
// squares of its quads in ascending order, x y z w inside a quad, every square and every sum in fp64 with contraction off.  The 16-byte
// loop and the scalar loop differ in how a quad is loaded and in nothing else, and both take pending slabs through slab_sum, so the
// partial of a block does not depend on where the gradient came from.  Block tree: __shfl_down by 32, 16, .. 1 in each wave, then
// ((w0 + w1) + w2) + w3.  One fp64 partial per block, at [segment * kNormBlocks + block].  This indexing is the kernel's own, which is
// why it does not go through segment_walk.
// Where a segment has pending slabs their sum is written to the gradient buffer (t.dst here), which the apply kernel then reads.
constexpr int kNormBlocks = 64;
constexpr int kNormMaxPartials = 16 * kNormBlocks;
struct ClipRecord {            // of the last clipped-mode apply / since clipping was switched on; written by one thread of the apply kernel
    double norm, coef;
    unsigned long long applies, clipped;
};
struct ClipArgs {
    const double* partials;    // grad_norm_kernel's, npart of them
    int npart;
    double max_norm, abs_scale;
    ClipRecord* rec;
};
__device__ __forceinline__ double sq_add(double acc, float g) {
#pragma clang fp contract(off)
    const double x = (double)g;
    const double x2 = x * x;
    return acc + x2;
}
__global__ __launch_bounds__(256) void grad_norm_kernel(SegTable t, double* __restrict__ partials) {
    const int sgm = (int)blockIdx.y;
    if (sgm >= t.nseg) return;
    float* out = t.dst[sgm];
    const float* s = t.src[sgm];
    const int nslabs = t.nslabs[sgm];
    const long long len = t.len[sgm], st = t.stride[sgm];
    const long long nq = (len + 3) >> 2;
    const long long step = (long long)kNormBlocks * 256;
    double acc = 0.0;
    if (t.vec4[sgm]) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += step) {
            float4 g;
            if (nslabs <= 0) g = s4[q];
            else { g = slab_sum(s4, nslabs, st >> 2, q); o4[q] = g; }
            acc = sq_add(sq_add(sq_add(sq_add(acc, g.x), g.y), g.z), g.w);
        }
    } else {
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += step) {
            const long long i0 = q << 2, i1 = i0 + 4 < len ? i0 + 4 : len;
            for (long long i = i0; i < i1; ++i) {
                float g;
                if (nslabs <= 0) g = s[i];
                else { g = slab_sum(s, nslabs, st, i); out[i] = g; }
                acc = sq_add(acc, g);
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[sgm * kNormBlocks + (int)blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// The coefficient, by every block of the apply kernel for itself: the partials added in index order by one thread, in fp64.  `writer`
// (one block of the grid) also leaves norm and c in the record and bumps its counters: plain stores, one writer, launches in stream order.
__device__ __forceinline__ float clip_coef(const ClipArgs& C, bool writer) {
    __shared__ double sp[kNormMaxPartials];
    __shared__ float sc;
    for (int i = (int)threadIdx.x; i < C.npart; i += (int)blockDim.x) sp[i] = C.partials[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0;
        for (int i = 0; i < C.npart; ++i) S += sp[i];
        const double norm = C.abs_scale * sqrt(S);
        const double q = C.max_norm / (norm + 1e-6);
        const float c = (float)(q > 1.0 ? 1.0 : q);
        sc = c;
        if (writer) {
            C.rec->norm = norm;
            C.rec->coef = (double)c;
            C.rec->applies += 1;
            if (c < 1.0f) C.rec->clipped += 1;
        }
    }
    __syncthreads();
    return sc;
}
__device__ __forceinline__ float clip_mul(float a, float c) {
#pragma clang fp contract(off)
    return a * c;
}
// SGD: p -= fl32(fl32(lr grad_scale) c) g;  Adam: g' = fl32(fl32(grad_scale) c) g.  c == 1: the products are exact, the bits those of the
// unclipped kernels.  The same walk and the same steps with the scaled factor; the table has no pending slabs left (grad_norm_kernel
// summed them into the gradient buffer), so the slab loops are compiled out.
__global__ void sgd_segments_clip_kernel(SegTable t, float alpha0, ClipArgs C) {
    const float alpha = clip_mul(alpha0, clip_coef(C, blockIdx.x == 0 && blockIdx.y == 0));
    segment_walk<false>(XQ_GRID_X, t, SgdStep{alpha});
}
__global__ void adam_segments_clip_kernel(SegTable t, AdamArgs A, ClipArgs C) {
    A.gs = clip_mul(A.gs, clip_coef(C, blockIdx.x == 0 && blockIdx.y == 0));
    segment_walk<false>(XQ_GRID_X, t, AdamStep{A}, A.m, A.v);
}
__global__ void sgd_segments_clip_soft_kernel(SegTable t, float alpha0, ClipArgs C, SoftArgs Z) {
    const float alpha = clip_mul(alpha0, clip_coef(C, blockIdx.x == 0 && blockIdx.y == 0));
    segment_walk<false, true>(XQ_GRID_X, t, SgdStep{alpha}, nullptr, nullptr, &Z);
}
__global__ void adam_segments_clip_soft_kernel(SegTable t, AdamArgs A, ClipArgs C, SoftArgs Z) {
    A.gs = clip_mul(A.gs, clip_coef(C, blockIdx.x == 0 && blockIdx.y == 0));
    segment_walk<false, true>(XQ_GRID_X, t, AdamStep{A}, A.m, A.v, &Z);
}

// The soft target update over a whole buffer (xq_dqn_soft_update_target; behind an apply whose target net may differ from the online net
// outside the TD segments): t[i] = soft_elem(tau, p[i], t[i]) for i < n, and the bf16 shadow t_bf[i] (nullptr: none) for i < n_bf — the
// shadow covers the weights only.  Grid-stride; vec != 0 (p, t 16-byte and t_bf 8-byte aligned): quads as 16-byte loads and stores, the
// up to three elements left by one thread each; the bits are those of the scalar rule either way.
__global__ __launch_bounds__(256) void soft_target_kernel(const float* __restrict__ p, float* __restrict__ t, uint16_t* __restrict__ t_bf,
                                                          long long n, long long n_bf, float tau, int vec) {
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    long long done = 0;
    if (vec) {
        const long long nq = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        float4* t4 = reinterpret_cast<float4*>(t);
        for (long long q = first; q < nq; q += stride) {
            const float4 o = soft_elems(tau, p4[q], t4[q]);
            t4[q] = o;
            const long long i0 = q << 2;
            if (t_bf) {
                if (i0 + 4 <= n_bf) store_bf16(t_bf, q, o);
                else {
                    const float e[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (i0 + k < n_bf) t_bf[i0 + k] = bf16_bits(e[k]);
                }
            }
        }
        done = nq << 2;
    }
    for (long long i = done + first; i < n; i += stride) {
        const float o = soft_elem(tau, p[i], t[i]);
        t[i] = o;
        if (t_bf && i < n_bf) t_bf[i] = bf16_bits(o);
    }
}

}  // namespace xq
