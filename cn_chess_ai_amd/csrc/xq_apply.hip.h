// xq_apply.hip.h — from partial sums to parameters: the ordered slab reduction, the segment table and its one walk for every optimizer, the Q head
// finish, the bf16 shadow stores, the SGD step (updateWeightsBiasesKernel dqn.cu:310-319, batched), Adam, clipping by the global norm, the soft target
// update.  (kernel half of xq_dqn.hip; included by xq_dqn.hip behind xq_tail.hip.h, inside namespace xq; needs xq_gemm.hip.h for bf16_bits)
#pragma once

namespace xq {

// ---- ordered slab sums and the segment walk of the optimizers ------------------------------------------------------------------------
// THE order in which partial-sum slabs are added, stated once: four chains z = j, j + 4, .. (leftover slabs continue chain 0), then
// (s0 + s1) + (s2 + s3).  T = float or float4 (element-wise: a quad has the bits of its four elements summed one by one).  Everything
// that promises "the bits of reduce_slabs_kernel" calls this; colsum_final_kernel (xq_tail.hip.h) spells the same order across four lanes.
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
