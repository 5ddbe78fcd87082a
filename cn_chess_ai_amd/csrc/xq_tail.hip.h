// xq_tail.hip.h — the gradient tail of a TD step: output-layer and bias gradients as ordered sums (out_grad_block, the column sums), the dense
// output delta, and the fused launches that carry the blocks of several kernels (td_tail_kernel).  In front of it: xq_td.hip.h (the TD rule);
// behind it: xq_apply.hip.h (slab sums, optimizers).  (kernel half of xq_dqn.hip; included by xq_dqn.hip only, inside namespace xq)
#pragma once

namespace xq {

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
    // grid order: [l0][l0 cold rows][grad][delta][out][colsum][sel]; n_* = blocks of each part (0 = absent)
    int n_l0, n_grad, n_delta, n_out, n_colsum, n_sel, n_l0cold;
    GemmArgs grad;  int grad_gx, grad_gy;          // 64x64 tiles: grid (gx, gy, splits)
    GemmArgs delta; int delta_gx;                  // grid (gx, gy, 1)
    const int32_t* og_act; const float* og_dsc; const float* og_alast; int og_n, og_H, og_chunk; float* og_partial;   // grid (24, chunks)
    const uint32_t* l0_boards; const float* l0_delta; int l0_n, l0_H, l0_HS, l0_chunk, l0_nsets, l0_nch; float* l0_partial;   // (90, nch, H / HS)
    const uint16_t* l0_planes; long long l0_plane_stride; int l0_kpad, l0_ncb;      // != nullptr: the matrix-pipe form on the packed hot rows,
    const uint16_t* l0_sel;                        // grid (3, H / 32, nch) ... and its selector half-words (xq_l0grad.hip.h)
    const L0HotTable* l0_hot;                      // hot / cold rows (xq_l0hot.h); the cold rows: (kL0ColdParts, nch) blocks behind the hot ones
    const uint16_t* l0_cold_list; const int* l0_cold_cnt;
    const uint32_t* sel_boards; int sel_n, sel_kpad; uint16_t* sel_out;             // TAIL_SEL: those half-words being made, 64 samples per block
    uint16_t* sel_cold_list; int* sel_cold_cnt;    // ... with the cold-occurrence lists
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
                int rest = b / a.l0_ncb, cb = b % a.l0_ncb, sqg = rest % kL0HotGroups, ch = rest / kL0HotGroups;
                if ((a.l0_nch & 7) == 0) { ch = b % a.l0_nch; rest = b / a.l0_nch; cb = rest % a.l0_ncb; sqg = rest / a.l0_ncb; }
                l0_grad_mfma_block<0, true>(a.l0_sel, a.l0_planes, a.l0_plane_stride, a.l0_kpad, a.l0_H, a.l0_chunk, a.l0_partial, sqg, cb, ch,
                                             reinterpret_cast<unsigned char*>(tail_smem), a.l0_hot);
                return;
            }
            const int per = kSquares * a.l0_nch;
            l0_grad_block(a.l0_boards, a.l0_delta, a.l0_n, a.l0_H, a.l0_HS, a.l0_chunk, a.l0_nsets, a.l0_partial, b % per, a.l0_nch, b / per, tail_smem);
            return;
        }
        b -= a.n_l0;
        if (L0MFMA) {                             // the rows the matrix-pipe blocks above leave out: short blocks (stores of zeros, in play)
            if (b < a.n_l0cold) {
                l0_cold_block(a.l0_hot, a.l0_cold_list, a.l0_cold_cnt, a.l0_delta, a.l0_H, a.l0_chunk, a.l0_partial, b / kL0ColdParts,
                              b % kL0ColdParts, kL0ColdParts);
                return;
            }
            b -= a.n_l0cold;
        }
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
        if (b < a.n_sel) {
            l0_sel_block(a.sel_boards, a.sel_n, a.sel_kpad, a.sel_out, b, reinterpret_cast<uint32_t*>(tail_smem), a.l0_hot, a.sel_cold_list,
                         a.sel_cold_cnt);
            return;
        }
    }
}

}  // namespace xq
