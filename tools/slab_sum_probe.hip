// tools/slab_sum_probe.hip — the ordered sums of xq_apply.hip.h (slab_sum through reduce_slabs_kernel, sgd_segments_kernel stepping and
// reduce_only, adam_segments_kernel; the same chains over rows in colsum_partial_kernel of xq_tail.hip.h) bit for bit against host loops that spell the order in
// plain C++: four chains z = j, j + 4, .., leftover terms into chain 0, then (s0 + s1) + (s2 + s3).  The kernels may load their terms
// whenever they like; the bits may not move.
//   slabs:    nslabs {1,2,3,4,5,7,8,9,15,16,17,31,32,33,63,64,65} x len {1,3,4,5,252,256,257,1028} x stride % 4 {0,1} x base {16-byte
//             aligned, off by one float}; the eight lengths are the eight segments of one table.  Every table runs three times: quads where
//             the alignment rule of seg_grid allows them, scalar everywhere, and a one-block grid (the walk's loop iterates).
//   columns:  n {64,65,127,128,129,1024} x C {1,63,64,65,256}, ld = C + 3, R and rows_per as bias_grads sets them; and two shapes with
//             more than 32 rows to a thread (a whole batch and a part).
// Inputs: seeded, exponents mixed over 2^-12 .. 2^12, with -0.0f and denormals among them.
// Negative control (host only): every slab shape is also summed in plain ascending order; a shape with nslabs >= 5 in which no element
// tells the two orders apart fails the probe — such inputs could not tell one order from another.
// Build the host half with contraction off (the device half keeps the library's default); where the device contracts (SGD's w - alpha g) the host says std::fmaf:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Xarch_host -ffp-contract=off -I include -o tools/_build/slab_sum_probe tools/slab_sum_probe.hip
// Usage: slab_sum_probe [--host]      (--host: references and control only, no device call: the form to run under a host sanitizer)
// Prints "slab_sum_probe: mismatches N" last; exit status 0 only if N == 0 and the control held.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include <random>
#include "../cn_chess_ai_amd/csrc/xq_internal.h"
#include "../cn_chess_ai_amd/csrc/xq_gemm.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_screen.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_gemm_dma.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_l0grad.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_l0.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_tail.hip.h"        // colsum_partial_kernel (and what its fused launch needs, above)
#include "../cn_chess_ai_amd/csrc/xq_apply.hip.h"
using namespace xq;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

// ---- the order, in plain C++ ----
static float chains_sum(const float* p, int n, long long st) {          // terms p[z * st], z < n
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int z = 0;
    for (; z + 3 < n; z += 4) {
        s0 = s0 + p[(long long)z * st];
        s1 = s1 + p[(long long)(z + 1) * st];
        s2 = s2 + p[(long long)(z + 2) * st];
        s3 = s3 + p[(long long)(z + 3) * st];
    }
    for (; z < n; ++z) s0 = s0 + p[(long long)z * st];
    return (s0 + s1) + (s2 + s3);
}
static float ascending_sum(const float* p, int n, long long st) {
    float s = 0.f;
    for (int z = 0; z < n; ++z) s = s + p[(long long)z * st];
    return s;
}
static float sgd_host(float w, float alpha, float g) { return std::fmaf(-alpha, g, w); }     // v_pk_fma_f32 .. neg_lo
static float adam_host(const AdamArgs& A, float p, float g, float& m, float& v) {           // adam_elem, operation for operation
    const float gp = A.gs * g;
    const float mg = A.omb1 * gp;
    m = std::fmaf(A.b1, m, mg);
    const float vg = (A.omb2 * gp) * gp;
    v = std::fmaf(A.b2, v, vg);
    const float den = std::fmaf(std::sqrt(v), A.rbc2, A.eps);
    const float q = m / den;
    return std::fmaf(-A.a, q, p);
}

// ---- inputs ----
static float mixed(std::mt19937& rng) {
    const uint32_t r = rng();
    const uint32_t kind = r & 15u;
    if (kind == 0) return -0.0f;
    if (kind == 1) { uint32_t u = (rng() & 0x007fffffu) | (r & 0x80000000u); float f; memcpy(&f, &u, 4); return f; }     // a denormal
    const int e = (int)((r >> 4) % 25u) - 12;
    const float mant = 1.0f + (float)(rng() & 0xffffffu) / 16777216.0f;
    return std::ldexp((r & 0x80000000u) ? -mant : mant, e);
}
static bool same_bits(float a, float b) { uint32_t x, y; memcpy(&x, &a, 4); memcpy(&y, &b, 4); return x == y; }

static const int kNslabs[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65};
static const int kLens[] = {1, 3, 4, 5, 252, 256, 257, 1028};
enum { kNL = 8, kGuard = 8 };

// One table: the eight lengths as eight segments, every array in one arena so that one copy moves it.  Offsets in floats.
struct Seg { long long len, stride, slabs, d, m, v; };
struct Table {
    int nslabs, smod, off;
    Seg seg[kNL];
    long long total, state_total;
    std::vector<float> arena;          // slabs, parameters (with guard floats behind them), Adam m and v
    std::vector<float> g;              // host: the ordered sums, per segment back to back (offset = seg.m - seg[0].m)
};
// the control: elements of segment k whose ascending sum has other bits than the four-chain sum
static long long control_differs(const Table& T, int k) {
    const Seg& s = T.seg[k];
    long long c = 0;
    for (long long i = 0; i < s.len; ++i)
        if (!same_bits(ascending_sum(&T.arena[s.slabs + i], T.nslabs, s.stride), T.g[(s.m - T.seg[0].m) + i])) ++c;
    return c;
}
static Table make_table(int nslabs, int smod, int off, uint32_t seed) {
    Table T; T.nslabs = nslabs; T.smod = smod; T.off = off;
    long long at = 0;
    auto take = [&](long long count) { at = (at + 3) & ~3LL; const long long o = at + off; at = o + count; return o; };   // 16-byte aligned + off
    for (int k = 0; k < kNL; ++k) {
        Seg& s = T.seg[k];
        s.len = kLens[k]; s.stride = ((s.len + 3) & ~3LL) + smod;
        s.slabs = take((long long)nslabs * s.stride);
        s.d = take(s.len + kGuard);
    }
    // Adam's state is laid out like the gradient buffer: one array, segment k at state_off[k] (a multiple of 4 + off)
    long long so = 0;
    const long long mbase = (at + 3) & ~3LL;
    for (int k = 0; k < kNL; ++k) { T.seg[k].m = mbase + so + off; so += (T.seg[k].len + 3) & ~3LL; }
    T.state_total = so + 4;
    const long long vbase = mbase + T.state_total;
    for (int k = 0; k < kNL; ++k) T.seg[k].v = vbase + (T.seg[k].m - mbase);
    T.total = vbase + T.state_total;
    T.arena.assign((size_t)T.total, 0.f);
    std::mt19937 rng(seed);
    T.g.assign((size_t)so, 0.f);
    for (int k = 0; k < kNL; ++k) {
        const Seg& s = T.seg[k];
        // The slabs of a segment are drawn again (the next values of the same stream; at most 64 times) while the control below cannot
        // tell the orders apart: with one to five elements a single draw often rounds alike both ways.  What decides is the host's two
        // sums alone, never a result of the device.
        for (int draw = 0; draw < 64; ++draw) {
            for (long long i = 0; i < (long long)nslabs * s.stride; ++i) T.arena[s.slabs + i] = mixed(rng);
            for (long long i = 0; i < s.len; ++i) T.g[(s.m - T.seg[0].m) + i] = chains_sum(&T.arena[s.slabs + i], nslabs, s.stride);
            if (nslabs < 5 || control_differs(T, k) > 0) break;
        }
        for (long long i = 0; i < s.len + kGuard; ++i) T.arena[s.d + i] = mixed(rng);
        for (long long i = 0; i < s.len; ++i) { T.arena[s.m + i] = 0.125f * mixed(rng); T.arena[s.v + i] = std::fabs(mixed(rng)); }
    }
    return T;
}

// ---- column sums ----
struct ColShape { int n, C, R, rows_per; };
static void colsum_host(const std::vector<float>& X, long long ld, const ColShape& S, std::vector<float>& work) {
    work.assign((size_t)S.R * S.C, 0.f);
    for (int by = 0; by < S.R; ++by) {
        const int r0 = by * S.rows_per, r1 = std::min(S.n, r0 + S.rows_per);
        for (int c = 0; c < S.C; ++c) {
            float red[4];
            for (int ty = 0; ty < 4; ++ty) {
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                int r = r0 + ty;
                for (; r + 12 < r1; r += 16) {
                    s0 = s0 + X[(long long)r * ld + c];
                    s1 = s1 + X[(long long)(r + 4) * ld + c];
                    s2 = s2 + X[(long long)(r + 8) * ld + c];
                    s3 = s3 + X[(long long)(r + 12) * ld + c];
                }
                for (; r < r1; r += 4) s0 = s0 + X[(long long)r * ld + c];
                red[ty] = (s0 + s1) + (s2 + s3);
            }
            work[(size_t)by * S.C + c] = (red[0] + red[1]) + (red[2] + red[3]);
        }
    }
}

static long long g_bad = 0;
static void report(const char* what, int nslabs, int smod, int off, int pass, long long len, long long bad) {
    if (bad) printf("MISMATCH %s: nslabs %d stride%%4 %d base+%d pass %d len %lld: %lld elements\n", what, nslabs, smod, off, pass, len, bad);
    g_bad += bad;
}

int main(int argc, char** argv) {
    const bool host_only = argc > 1 && !strcmp(argv[1], "--host");
    const uint32_t seed0 = 20260;
    AdamArgs A; memset(&A, 0, sizeof A);
    A.b1 = 0.9f; A.omb1 = (float)(1.0 - 0.9); A.b2 = 0.999f; A.omb2 = (float)(1.0 - 0.999); A.eps = 1e-8f;
    A.a = (float)(1e-3 / (1.0 - std::pow(0.9, 3.0))); A.rbc2 = (float)(1.0 / std::sqrt(1.0 - std::pow(0.999, 3.0))); A.gs = 1.0f / 64;
    const float alpha = 0.001f / 64;
    long long control_fail = 0, tables = 0, launches = 0;
    float* dev = nullptr;
    size_t dev_floats = 0;
    std::vector<float> back;
    int ti = 0;
    for (int nslabs : kNslabs) for (int smod = 0; smod < 2; ++smod) for (int off = 0; off < 2; ++off, ++ti) {
        Table T = make_table(nslabs, smod, off, seed0 + 977u * (uint32_t)ti);
        ++tables;
        if (nslabs >= 5)
            for (int k = 0; k < kNL; ++k)
                if (control_differs(T, k) == 0) {
                    printf("CONTROL: nslabs %d stride%%4 %d base+%d len %lld: ascending order gives the same bits in every element\n", nslabs, smod, off, T.seg[k].len);
                    ++control_fail;
                }
        if (host_only) continue;
        if ((size_t)T.total > dev_floats) {
            if (dev) CK(hipFree(dev));
            dev_floats = (size_t)T.total + 4096;
            CK(hipMalloc(&dev, dev_floats * sizeof(float)));
        }
        back.resize((size_t)T.total);
        auto upload = [&]() { CK(hipMemcpy(dev, T.arena.data(), (size_t)T.total * 4, hipMemcpyHostToDevice)); };
        auto download = [&]() { CK(hipDeviceSynchronize()); CK(hipMemcpy(back.data(), dev, (size_t)T.total * 4, hipMemcpyDeviceToHost)); };
        auto guards_ok = [&](int k) {
            long long bad = 0;
            for (int i = 0; i < kGuard; ++i) if (!same_bits(back[T.seg[k].d + T.seg[k].len + i], T.arena[T.seg[k].d + T.seg[k].len + i])) ++bad;
            return bad;
        };
        // reduce_slabs_kernel: one launch per segment, out = the parameter array
        upload();
        for (int k = 0; k < kNL; ++k) {
            const Seg& s = T.seg[k];
            hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((s.len + 255) / 256)), dim3(256), 0, 0, dev + s.slabs, nslabs, s.stride, s.len, dev + s.d);
            ++launches;
        }
        CK(hipGetLastError());
        download();
        for (int k = 0; k < kNL; ++k) {
            const Seg& s = T.seg[k];
            long long bad = guards_ok(k);
            for (long long i = 0; i < s.len; ++i) if (!same_bits(back[s.d + i], T.g[(s.m - T.seg[0].m) + i])) ++bad;
            report("reduce_slabs_kernel", nslabs, smod, off, 0, s.len, bad);
        }
        // the segment walk: pass 0 quads where seg_grid's rule allows, pass 1 scalar everywhere, pass 2 as pass 0 on a one-block grid
        for (int pass = 0; pass < 3; ++pass) {
            SegTable t; memset(&t, 0, sizeof t);
            t.nseg = kNL;
            long long mx = 0;
            bool any4 = false;
            for (int k = 0; k < kNL; ++k) {
                const Seg& s = T.seg[k];
                t.dst[k] = dev + s.d; t.src[k] = dev + s.slabs; t.len[k] = s.len; t.nslabs[k] = nslabs; t.stride[k] = s.stride;
                t.state_off[k] = s.m - T.seg[0].m;
                const bool v4 = pass != 1 && off == 0 && (s.len & 3) == 0 && (s.stride & 3) == 0 && (t.state_off[k] & 3) == 0;
                t.vec4[k] = v4; any4 |= v4;
                mx = std::max(mx, v4 ? s.len / 4 : s.len);
            }
            if (pass == 1 && !(off == 0 && smod == 0)) continue;          // (pass 0 was scalar everywhere already)
            (void)any4;
            const unsigned bx = pass == 2 ? 1u : (unsigned)((mx + 255) / 256);
            for (int kern = 0; kern < 3; ++kern) {                       // 0 SGD step, 1 SGD table with reduce_only, 2 Adam
                upload();
                t.reduce_only = kern == 1;
                AdamArgs Ad = A; Ad.m = dev + T.seg[0].m; Ad.v = dev + T.seg[0].v;
                if (kern == 2) hipLaunchKernelGGL(adam_segments_kernel, dim3(bx, kNL), dim3(256), 0, 0, t, Ad);
                else hipLaunchKernelGGL(sgd_segments_kernel, dim3(bx, kNL), dim3(256), 0, 0, t, kern == 1 ? 0.f : alpha);
                CK(hipGetLastError());
                ++launches;
                download();
                for (int k = 0; k < kNL; ++k) {
                    const Seg& s = T.seg[k];
                    long long bad = guards_ok(k);
                    for (long long i = 0; i < s.len; ++i) {
                        const float g = T.g[(s.m - T.seg[0].m) + i], w = T.arena[s.d + i];
                        float m = T.arena[s.m + i], v = T.arena[s.v + i];
                        const float want = kern == 0 ? sgd_host(w, alpha, g) : kern == 1 ? g : adam_host(A, w, g, m, v);
                        if (!same_bits(back[s.d + i], want)) ++bad;
                        if (!same_bits(back[s.m + i], m) || !same_bits(back[s.v + i], v)) ++bad;      // SGD: the state is left alone
                    }
                    report(kern == 0 ? "sgd_segments_kernel" : kern == 1 ? "sgd_segments_kernel reduce_only" : "adam_segments_kernel", nslabs, smod, off, pass, s.len, bad);
                }
            }
        }
    }
    // column sums
    std::vector<ColShape> shapes;
    for (int n : {64, 65, 127, 128, 129, 1024}) for (int C : {1, 63, 64, 65, 256}) {
        ColShape S; S.n = n; S.C = C; S.R = std::max(1, std::min(64, n / 64)); S.rows_per = (n + S.R - 1) / S.R;
        shapes.push_back(S);
    }
    shapes.push_back(ColShape{301, 65, 2, 151});       // 38 / 37 rows to a thread: a whole batch of 32 and a part
    shapes.push_back(ColShape{520, 64, 2, 260});       // 65 rows: two whole batches and one row
    long long col_launches = 0;
    for (size_t si = 0; si < shapes.size(); ++si) {
        const ColShape& S = shapes[si];
        const long long ld = S.C + 3;
        std::mt19937 rng(seed0 + 31u * (uint32_t)si + 7u);
        std::vector<float> X((size_t)S.n * ld), want;
        for (auto& x : X) x = mixed(rng);
        colsum_host(X, ld, S, want);
        if (host_only) continue;
        float *dX, *dW;
        const size_t wcount = (size_t)S.R * S.C + kGuard;
        CK(hipMalloc(&dX, X.size() * 4)); CK(hipMalloc(&dW, wcount * 4));
        CK(hipMemcpy(dX, X.data(), X.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemset(dW, 0x5a, wcount * 4));
        ColsumJobs J; memset(&J, 0, sizeof J);
        J.X[0] = dX; J.ld[0] = ld; J.C[0] = S.C; J.dst[0] = nullptr; J.poff[0] = 0;
        J.njobs = 1; J.n = S.n; J.rows_per = S.rows_per; J.R = S.R; J.work = dW; J.wld = S.C;
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((S.C + 63) / 64, S.R, 1), dim3(256), 0, 0, J);
        CK(hipGetLastError());
        ++col_launches;
        std::vector<float> got(wcount);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(got.data(), dW, wcount * 4, hipMemcpyDeviceToHost));
        long long bad = 0;
        for (size_t i = 0; i < want.size(); ++i) if (!same_bits(got[i], want[i])) ++bad;
        for (int i = 0; i < kGuard; ++i) { uint32_t u; memcpy(&u, &got[want.size() + i], 4); if (u != 0x5a5a5a5au) ++bad; }
        if (bad) printf("MISMATCH colsum_partial_kernel: n %d C %d R %d rows_per %d: %lld elements\n", S.n, S.C, S.R, S.rows_per, bad);
        g_bad += bad;
        CK(hipFree(dX)); CK(hipFree(dW));
    }
    if (dev) CK(hipFree(dev));
    printf("slab_sum_probe: %lld slab tables x %d lengths, %zu column shapes, %lld + %lld launches%s; control failures %lld\n", tables, (int)kNL,
           shapes.size(), launches, col_launches, host_only ? " (host only: nothing launched)" : "", control_fail);
    printf("slab_sum_probe: mismatches %lld\n", g_bad);
    return (g_bad || control_fail) ? 1 : 0;
}
