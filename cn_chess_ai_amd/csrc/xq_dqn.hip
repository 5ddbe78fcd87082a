// xq_dqn.hip — DQN = online + target NeuralNetwork on the CDNA4 matrix cores (fp32), batched.
//
// Reference: include/dqn.h:42-116, src/dqn.cpp, src/dqn.cu (fp64, batch 1, one thread per output neuron, a
// cudaMalloc/H2D/launch/sync/D2H round trip per layer).  Here the whole TD step of a minibatch stays in HBM:
//   layer 0      : the 1260-wide one-hot input (chessai.cpp:268-289) is never built — rows of W0^T are gathered by
//                  (square, piece) straight from the packed board (<= 32 rows of 1 KB per sample, L2-resident);
//   hidden / Q   : xq_gemm.hip.h MFMA GEMMs with fused bias+tanh;
//   max_a' Q(s') : the 8100-wide output GEMM never writes Q — its epilogue reduces max(z) per row (tanh is monotone);
//   backward     : the TD target equals Q(s) except at action.to < 90 (chessai.cpp:122-128), so the output delta
//                  lives in columns 0..95: delta GEMM with K = 96, weight-gradient GEMM with M = 96;
//   layer-0 grad : one-hot^T x delta as per-(square, piece) segmented sums of delta rows (ordered, in LDS accumulators);
//   reductions over the batch are split-K into slabs + an ordered slab sum: bitwise reproducible, no float atomics.
// Device parameter layout (one flat fp32 buffer per net): [W0^T (L0 x L1)] [W_1 .. W_out, reference layout
// row-major [out][in], concatenated] [b_0 .. b_out].  Keeping layers >= 1 in the reference's flat order lets the
// bug-compatible hidden delta (dqn.cu:406-423 as written: wrong stride, reads across layer boundaries) be expressed
// as the same GEMM with a different base/leading dimension.
// The forward half is described once too: layer 0 (l0_select_forward with kept sums, l0_forward grouped) and one function per hidden
// product (hidden_bf16_dma, hidden_bf16_tile, hidden_f32_head, hidden_f32_walk, the fp32 tile kernel), each with its own shape test,
// operands, accounting and launch; hidden_forward picks one, chain_boards is the argument checks, the layer-0 call and the loop.
// The gradient half of a TD step is described once (plan_gradients, out_gradient, hidden_weight_gradient, hidden_bias_gradients,
// l0_gradient) and emitted in two orders: side_gradients (two streams) and tail_launches (fused grids, TailGrid).
// The screened max pass is described once as well: xq::Screen owns its buffers, counters and guard, and plans each step's part of it
// (ScreenPlan in TdStep); qmax_screened is the launches.  What a write of the parameters makes stale is described once: params_written,
// the one place that touches params_version, the screen's kept rows, the select chain's kept sums and tgt_rest_synced.
// This file = the handle (struct xq_dqn) + host orchestration + the C ABI; the kernels live in xq_l0.hip.h (layer-0 gathers and
// segmented sums), xq_td.hip.h (the TD rule: fold, target, delta, record, priority), xq_tail.hip.h (gradient sums, fused launches),
// xq_apply.hip.h (slab sums, segment walk, optimizers, clipping, soft target), xq_refine.hip.h (screening pass 2), xq_l0grad.hip.h (layer-0
// gradient on the matrix pipe), xq_gemm*.hip.h and xq_screen.hip.h (matrix-pipe products), xq_nstep.hip.h and
// xq_stage.hip.h (staging of n-step, mirrored, colour-swapped and mover-view batches), xq_legal.hip.h (the legal-move bootstrap, on the rules engine of xq_rules.hip.h).
#include "xq_internal.h"
#include <hip/hip_ext.h>
#include "xq_gemm.hip.h"
#include "xq_screen.hip.h"
#include "xq_gemm_dma.hip.h"
#include "xq_l0grad.hip.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <mutex>
#include <random>
#include <unordered_map>

struct TdStep; struct ScreenPlan;
namespace xq {
struct TailArgs; struct ClipRecord; struct TdStatsRecord; struct ShadowJob;
// Exact screening of max_a' Q(s', a') (xq_dqn_set_qmax_mode), state and host logic: bf16 copies of the output-layer weights
// and of the last hidden activations of s', the two screening partial arrays, the largest row norm of the weights, counters, the guard
struct Screen {
    int mode = XQ_QMAX_FULL;
    int refine_stage = -1;                      // xq_dqn_set_refine_stage: -1 by the counters (stage_whole), 0 never, 1 whenever it fits
    DevBuf<uint16_t> wb;                        // [round_up(nout,128)][hlast] (rows >= nout zero)
    DevBuf<uint16_t> ab;                        // [round_up(cap,512)][hlast]: row-major, or B-fragment order for screen_top2_kernel
    DevBuf<float> p1, p2;                       // [4*tiles_m][round_up(cap,512)]
    DevBuf<float> R, na;                        // [chunks][round_up(cap,512)] per-range maxima, [round_up(cap,512)] ||bf16(a)||^2
    // bits of the largest row norm / largest |bias| of the output layer (non-negative floats order like unsigned): [0..1] rows 0..95 by
    // step parity, [2..3] their biases by step parity, [4] rows >= 96, [5] their biases.  Only rows 0..95 change under the TD rule
    // (xq_dqn_td_grads never touches the others), so the shadow of rows >= 96 and slots [4], [5] are kept from step to step:
    DevBuf<unsigned> wmax;
    int static_net = -1;                        // net whose rows >= 96 the shadow holds (-1: none — the next step converts everything)
    DevBuf<unsigned long long> stats;           // [refine blocks][2] running totals per block: candidate (sample, group) pairs, pairs recomputed as whole groups
    int stat_blocks = 0;                        // blocks the array (and its pinned copy) has room for
    unsigned long long carry[2] = {0, 0};       // totals of an array that was replaced by a larger one
    unsigned long long host_steps = 0, host_samples = 0;
    // guard: every kScreenCheckEvery screened steps the candidate counters are copied back asynchronously and evaluated kScreenCheckEvery
    // steps later; a net that leaves the screen too many candidates (outputs all within the bf16 bound of each other) gets the full
    // product for the next kScreenHoldSteps steps
    PinnedBuf<unsigned long long> guard_host;   // pinned copy of stats
    Event guard_ev;                             // created on first use (reserve)
    bool guard_pending = false;
    unsigned long long guard_samples = 0, guard_queued_at = 0;      // host_samples, host_steps when the pending copy was queued
    bool stage_whole = false;                   // the last counter window showed whole groups for many samples: the refine kernel is launched with the LDS of its
                                                // staged pass (145 KB: otherwise it would keep the select chain's blocks off its CUs for nothing — +3 us per step)
    unsigned long long seen[3] = {0, 0, 0};     // samples, pairs, whole groups at the last evaluation
    int hold = 0;                               // > 0: that many TD steps still run the full product
    bool rebase = false;                        // a hold began and `seen` has not been re-based since: the next copy decides nothing (guard_queue)
    unsigned long long fallbacks = 0;
    void set_mode(int m) { mode = m; hold = 0; }         // an explicit request starts with the screen switched on again
    void rows_rewritten(int net) { if (static_net == net) static_net = -1; }     // rows >= 96 of `net` are no longer what the shadow holds
    // (defined below the kernel headers, whose constants they use)
    int reserve(int NO, int Hl, int n, const void* params, const void* acts);
    void totals_of(const unsigned long long* h, unsigned long long sums[2]) const;  int totals(unsigned long long sums[2]) const;
    void guard_decide(const unsigned long long totals[2]);  int guard_tick(bool* screened);  int guard_queue(int n, hipStream_t s);
    int shadow_job(const xq_dqn* d, int sel_net, int parity, hipStream_t s, ShadowJob* shadow);
    int plan(xq_dqn* d, const TdStep& s, ScreenPlan* P);
};
// The staging batch of a TD step from a ring: what the staging kernels fill — nstep_assemble_kernel, mirror_stage_kernel,
// colour_swap_stage_kernel, mover_view_stage_kernel, in that order, the first one on gathering from the ring and every later one working
// in place — and the TD step then reads with the identity slot source
struct StageIo;
struct StagedBatch {
    enum : unsigned { kAssemble = 1u, kMirror = 2u, kColourSwap = 4u, kView = 8u };
    DevBuf<uint32_t> ns_boards, ns_next;
    DevBuf<int32_t> ns_action, ns_first;        // ns_first: the sampled slot
    DevBuf<float> ns_reward;                    // (behind the assembly: the n-step return)
    DevBuf<uint8_t> ns_done;
    DevBuf<int32_t> ns_m, ns_last;              // assembly: chain elements used, the slot whose next board was staged
    DevBuf<uint8_t> ns_flag, ns_cflag;          // mirror / colour swap: the row's flag
    DevBuf<uint8_t> ns_vflag, ns_vflag_next;    // view: the flags of s and of s'
    DevBuf<uint8_t> ns_side;                    // legal-move bootstrap: the side to move in the staged s'
    // the last TD step: its rows if it ran on this batch (else 0), the stages that filled it, whether a transform staged the side bytes
    struct Last { int rows = 0; unsigned stages = 0; bool sided = false; } last;
    int reserve(size_t rows) {                  // the columns every stage shares
        XQ_TRY(ns_boards.reserve(rows * kBoardWords));
        XQ_TRY(ns_next.reserve(rows * kBoardWords));
        for (DevBuf<int32_t>* b : {&ns_action, &ns_first}) XQ_TRY(b->reserve(rows));
        XQ_TRY(ns_reward.reserve(rows));
        return ns_done.reserve(rows);
    }
    StageIo io(const ReplayDev* ring) const;    // gather from `ring`, or (nullptr) the batch in place; defined below the kernel headers
};
}  // namespace xq
struct xq_dqn {
    int ns = 0, nl = 0;
    int L[XQ_MAX_LAYERS + 1] = {0};
    size_t nw = 0, nb = 0;
    size_t wo[XQ_MAX_LAYERS] = {0}, bo[XQ_MAX_LAYERS] = {0};
    double lr = 1e-3, gamma = 0.99;
    uint64_t seed = 0;
    xq::Stream stream;
    // side stream for work that is independent of the main chain inside one TD step (the s-chain forward runs beside the
    // s'-chain + column-max GEMM; the layer-0 gradient beside the other gradient GEMMs); `cur` = stream launches go to (OnStream)
    xq::Stream side;
    hipStream_t cur = nullptr;
    int ncu = 256;                              // compute units of the device (persistent-kernel grid = 2 per CU)
    xq::Event ev_fork, ev_join, ev_delta;
    xq::Event ev_qmax;                          // recorded behind the column-max GEMM of the last TD step (trainer: collect starts here)
    xq::DevBuf<float> params[2];
    uint64_t params_version = 0;                // ++ whenever an operation that rewrites parameters is queued (params_written; xq_trainer: is its `params` mark still current?)
    // bf16 Q-net (xq_dqn_set_precision): bf16 shadow of the WEIGHTS of both nets, same element order as params[] (biases stay fp32);
    // forward kernels read the shadow, the backward pass and the SGD step work on the fp32 master copy and refresh the shadow
    int precision = XQ_PRECISION_F32;
    xq::DevBuf<uint16_t> params_bf[2];
    xq::DevBuf<uint16_t> acts_bf[XQ_MAX_LAYERS];       // bf16 bits of acts[] (acts[] then holds the same, rounded, values in fp32)
    xq::DevBuf<uint16_t> tacts_bf[2];
    xq::DevBuf<uint16_t> t2acts_bf[2];
    xq::DevBuf<uint16_t> sel_acts_bf[XQ_MAX_LAYERS];
    xq::DevBuf<uint16_t> deltas_bf[XQ_MAX_LAYERS];     // XQ_PRECISION_BF16_FULL: the hidden deltas rounded to bf16 (operands of the backward products)
    xq::DevBuf<float> t2acts[2];                       // third forward chain of a Double-DQN step (s' on the target net)
    xq::DevBuf<int> partial_idx;                       // row index of each column-max partial (Double DQN)
    // workspaces sized for the largest batch seen (ensure_capacity)
    xq::DevBuf<float> acts[XQ_MAX_LAYERS];      // online hidden activations a_{l+1} = tanh(z_l), l = 0..nl-2
    xq::DevBuf<float> tacts[2];                 // ping-pong chain for s' / inference
    xq::DevBuf<float> deltas[XQ_MAX_LAYERS];    // delta_l of hidden layer l
    xq::DevBuf<float> dsc;                      // [cap] the one non-zero output delta of each TD sample
    xq::DevBuf<int32_t> act_mb;                 // [cap] action.to of each TD sample (gathered), -1 = empty slot
    xq::DevBuf<float> q90;                      // [cap][96]
    // second workspace for the action-select chain, so that it can run on its own stream beside a TD step
    xq::DevBuf<float> sel_acts[XQ_MAX_LAYERS];
    xq::DevBuf<float> sel_q90;
    // layer-0 sums of the select chain kept from ply to ply (xq_dqn_set_l0_derive, fp32 net): while the online weights do not change
    // — the plies of one update — the next ply's sums are the kept ones minus the rows of the squares that changed plus the rows of
    // what stands there now (l0_select_kernel); `boards` / `n` = whose boards the kept state belongs to.  One set per stream the chain
    // runs on — [0] the handle's stream (xq_dqn_select_q_dev), [1] any other (the trainer's collect stream) — like qh_slabs: a query on
    // the handle's stream neither races with collects in flight nor changes what their next ply derives from
    struct SelKeep {
        xq::DevBuf<float> z1;  xq::DevBuf<uint32_t> prev_boards;
        bool valid = false;  const uint32_t* boards = nullptr;  int n = 0;
        int calls = 0;  bool pays = false;                // select calls since the last parameter update; the last period had >= 2
    } sel_keep[2];
    void sel_invalidate() { sel_keep[0].valid = sel_keep[1].valid = false; }
    xq::DevBuf<float> qh_slabs[2];              // k-slabs of the select head (handle stream / any other stream)
    bool small_tiles = false;                   // force 64x64 GEMM tiles (<= 80 VGPRs: fits beside the persistent GEMM); written by SmallTiles alone
    bool l0_derive = false;                     // xq_dqn_set_l0_derive: layer-0 sums of s' from those of s (online TD rule, fp32 net)
    xq::Screen scr;                             // the screened max_a' Q(s', a') of a TD step (xq_dqn_set_qmax_mode)
    xq::DevBuf<float> partial;                  // row-max partials
    xq::DevBuf<float> zmax;  xq::DevBuf<int> zidx;  // [kReduceParts][cap] their reduction per sample (colmax_reduce_kernel)
    xq::DevBuf<float> qsa, yv, lossv;
    xq::DevBuf<uint32_t> gboards;               // [cap][12] boards of the current minibatch, gathered
    int last_n = 0;
    // gradients
    xq::DevBuf<float> grads_td;  size_t n_grads_td = 0;
    size_t g_w0 = 0, g_wh[XQ_MAX_LAYERS] = {0}, g_wout = 0, g_bh[XQ_MAX_LAYERS] = {0}, g_bout = 0;
    xq::DevBuf<float> grads_full;
    // optimizer of xq_dqn_apply_grads (xq_dqn_set_optimizer): Adam's first and second moments in the layout of grads_td, allocated on
    // the first switch to Adam; opt_t = Adam applies since the state was last reset
    int opt_kind = XQ_OPT_SGD;
    double opt_b1 = 0.9, opt_b2 = 0.999, opt_eps = 1e-8;
    uint64_t opt_t = 0;
    xq::DevBuf<float> adam_m, adam_v;
    // gradient clipping of xq_dqn_apply_grads (xq_dqn_set_grad_clip): 0 = off; the per-block partials of grad_norm_kernel and the
    // device record the apply kernel writes (norm, coefficient, counters), both allocated on the first switch-on
    double clip_max_norm = 0.0;
    xq::DevBuf<double> clip_partials;
    xq::DevBuf<xq::ClipRecord> clip_rec;
    // soft target update of xq_dqn_apply_grads (xq_dqn_set_target_tau): 0 = off, (0, 1) = theta- += tau (theta - theta-) in the apply
    // kernel, 1 = the hard copy behind every apply.  tgt_rest_synced: the target's parameters OUTSIDE the TD segments have the online
    // net's bits (a fixed point of the rule), so the apply kernel's walk over the TD segments is the whole update; written by
    // params_written alone (its table); while false, one whole-buffer kernel follows the apply instead
    double target_tau = 0.0;
    bool tgt_rest_synced = false;
    // TD loss of xq_dqn_td_grads* (xq_dqn_set_td_loss): squared, or Huber with kappa (loss_kappa32 = the float the kernels clamp at; +inf
    // allowed).  td_stats_rec: the record of td_error_stats_kernel, allocated by the first xq_dqn_td_error_stats
    int loss_kind = XQ_LOSS_SQUARED;
    double loss_kappa = 1.0;
    float loss_kappa32 = 1.0f;
    xq::DevBuf<xq::TdStatsRecord> td_stats_rec;
    xq::DevBuf<float> slabs;
    xq::DevBuf<float> slabs_l0;                 // layer-0 gradient partials
    // layer-0 gradient on the bf16 matrix pipe (xq_l0grad.hip.h): delta_0 as three bf16 planes, transposed [plane][column][sample]
    xq::DevBuf<uint16_t> l0_planes;
    xq::DevBuf<uint16_t> l0_sel;                // selector half-words of the minibatch's boards (xq_l0grad.hip.h)
    xq::DevBuf<uint16_t> l0_hot;                // the hot-row table (xq_l0hot.h), as built on the host
    xq::DevBuf<uint16_t> l0_cold_list;          // cold occurrences of the minibatch's boards, per 64 samples, and their counts
    xq::DevBuf<int> l0_cold_cnt;
    const xq::L0HotTable* hot() const { return reinterpret_cast<const xq::L0HotTable*>(l0_hot.p); }
    bool l0_split_done = false;                 // this step's layer-0 delta product wrote the planes in its epilogue
    bool l0_sel_done = false;                   // this step's selector words rode in an earlier fused launch
    bool l0_mfma = true;                        // xq_dqn_set_l0_grad_mode (default since round 5: xq_l0grad.hip.h)
    xq_comm* comm = nullptr;                    // xq_dqn_set_comm: bucketed RCCL all-reduce of the gradient buffer inside td_grads
    bool fused_apply = false;                   // xq_dqn_set_fused_apply: apply_grads may sum the partial-sum slabs itself
    // nslabs > 0: that many partial-sum slabs of a segment of the TD gradient wait at src, not yet summed into grads_td.  One slot per
    // segment of for_td_segments: layer 0 (its slabs are slabs_l0), the hidden weights, output rows 0..95 and their biases, the hidden
    // biases (rows of column sums, bias_grads).  Filled by the gradient half of a TD step, emptied by whatever sums them.
    struct PendingSlab { const float* src = nullptr; int nslabs = 0; long long stride = 0; };
    PendingSlab pend_w0, pend_hidden[XQ_MAX_LAYERS], pend_wout, pend_bout, pend_bh;
    xq::DevBuf<float> bias_work;
    // dense API scratch
    xq::DevBuf<float> xdense, qfull, tfull;
    xq::DevBuf<uint32_t> hb;                    // host-batch staging: boards, next boards
    xq::DevBuf<int32_t> ha;  xq::DevBuf<float> hr;  xq::DevBuf<uint8_t> hd;
    // the staging batch of a TD step from a ring (n-step returns, mirror, colour swap, mover view: DESIGN.md §4 "Staging pipeline")
    xq::StagedBatch staged;
    // legal-move bootstrap (xq_dqn_set_td_bootstrap): the k-slabs of the 96-row head product of s' (the selecting net's, then the target
    // net's of a Double-DQN step), the pre-activations legal_qmax_kernel leaves of them, the move count per row, the host batch's side
    // bytes.  legal_rows: rows of the last TD step if it was a legal one, else 0 (xq_dqn_last_legal)
    int bootstrap = XQ_BOOTSTRAP_ALL;
    xq::DevBuf<float> z96, z96_slabs;
    xq::DevBuf<int> legal_nmoves;
    xq::DevBuf<uint8_t> hside;                  // side bytes of the host batch (the staged batch's: staged.ns_side)
    int legal_rows = 0;
    // zero-sum (negamax) target (xq_dqn_set_zero_sum, DESIGN.md §4 "Zero-sum target"): the TD step's discount is -(float)gamma, the
    // n-step discounts alternate in sign, and a side without a move under the legal bootstrap bootstraps from -inf (tanh: -1)
    int zero_sum = 0;
    // mover view (xq_dqn_set_view, DESIGN.md §4 "Mover view"): a TD step from a ring stages view(s, mover) and view(s', next side) with
    // mover_view_stage_kernel, the last staging transform
    int view = XQ_VIEW_ABSOLUTE;
    xq::Profiler prof;
    // fused launches of the TD step's tail (td_tail_kernel): while `tail_open`, the launch helpers of the small fp32 GEMMs, the
    // output-layer / layer-0 segmented sums and the bias column sums append their blocks to `tail` instead of launching.  Written by
    // the scope objects TailGrid and LaunchNow alone
    xq::TailArgs* tail = nullptr;
    bool tail_open = false;
    bool td_tail = true;                        // xq_dqn_set_td_tail
    int exchange_overlap = -1;                  // xq_dqn_set_exchange_overlap: -1 auto (on when the communicator has more than one rank), 0, 1
    bool late_gate = false;                     // this TD step records ev_qmax behind its gradients (see tail_gradients)
    // xq_dqn_calibrate_exchange: mean duration of an all-reduce of the gradient buffer on this communicator, the threshold it was held
    // against and the start of the select chain chosen from the two (exchange_overlap == -1 only)
    bool exch_calibrated = false, exch_late = false;
    double exch_allreduce_us = 0.0, exch_threshold_us = 0.0;
    size_t tail_lds = 0;  double tail_flops = 0, tail_bytes = 0;

    // partial-sum slabs may stay unreduced until the apply kernel only when nothing (an all-reduce) reads the buffer in between
    bool fused() const { return fused_apply && comm == nullptr; }
    bool bf16() const { return precision != XQ_PRECISION_F32; }               // bf16 forward passes
    bool bf16_bwd() const { return precision == XQ_PRECISION_BF16_FULL; }     // ... and bf16 operands in the backward products
    uint16_t* wl_bf(int net, int l) const { return params_bf[net] + (l == 0 ? 0 : (size_t)L[0] * L[1] + (wo[l] - wo[1])); }
    float* w0t(int net) const { return params[net]; }
    float* wrest(int net) const { return params[net] + (size_t)L[0] * L[1]; }     // layers 1.. in reference flat order
    float* wl(int net, int l) const { return l == 0 ? w0t(net) : wrest(net) + (wo[l] - wo[1]); }
    float* bl(int net, int l) const { return params[net] + nw + bo[l]; }
    int nout() const { return L[nl]; }
    int hlast() const { return L[nl - 1]; }
};

namespace xq {

Profiler* dqn_profiler(xq_dqn* d) { return &d->prof; }
int dqn_fused_apply(const xq_dqn* d) { return d->fused_apply ? 1 : 0; }
int dqn_view(const xq_dqn* d) { return d->view; }
xq_comm* dqn_comm(const xq_dqn* d) { return d->comm; }
hipStream_t dqn_stream(xq_dqn* d) { return d->stream; }
void dqn_shape(const xq_dqn* d, int* n_in, int* n_out) { *n_in = d->L[0]; *n_out = d->nout(); }
hipEvent_t dqn_qmax_event(xq_dqn* d) { return d->ev_qmax; }
uint64_t dqn_params_version(const xq_dqn* d) { return d->params_version; }

struct ProfScope {
    Profiler& p; hipStream_t s; int h; double flops, bytes;
    // (while a fused tail launch is being assembled nothing is launched, so nothing is bracketed: TailGrid::launch has its own scope)
    // A launch on a stream that is neither the handle's nor its side stream belongs to the select chain of the self-play loop (the
    // trainer's collect stream): same kernels, other shapes, off the critical path — bracketed under "<name>@select".
    // attach: the scope is ONE kernel launch that takes start() / stop() as its own events (hipExtLaunchKernelGGL): kernel-exact time
    ProfScope(xq_dqn* d, const char* name, double fl, double by, bool attach = false) : p(d->prof), s(d->cur), flops(fl), bytes(by) {
        h = -1;
        if (!name || d->tail_open || !p.enabled) return;     // (no name: a launch that is not bracketed)
        if (d->cur != d->stream && d->cur != d->side) {
            char nm[48];
            snprintf(nm, sizeof nm, "%s@select", name);
            h = p.begin(nm, s, attach);
        } else {
            h = p.begin(name, s, attach);
        }
    }
    hipEvent_t start() const { return h >= 0 ? p.recs[h].a : nullptr; }
    hipEvent_t stop() const { return h >= 0 ? p.recs[h].b : nullptr; }
    ~ProfScope() { p.end(h, s, flops, bytes); }
};

// While one lives, the launch helpers launch — in front of the fused grid that is being assembled, if one is (TailGrid)
struct LaunchNow {
    xq_dqn* d; bool was_open;
    explicit LaunchNow(xq_dqn* d_) : d(d_), was_open(d_->tail_open) { d->tail_open = false; }
    ~LaunchNow() { d->tail_open = was_open; }
};
// While one lives, launches go to stream `s`
struct OnStream {
    xq_dqn* d; hipStream_t was;
    OnStream(xq_dqn* d_, hipStream_t s) : d(d_), was(d_->cur) { d->cur = s; }
    ~OnStream() { d->cur = was; }
};
// While one lives, the tile kernels take 64x64 tiles if `small` (the select chain beside a TD step)
struct SmallTiles {
    xq_dqn* d; bool was;
    SmallTiles(xq_dqn* d_, bool small) : d(d_), was(d_->small_tiles) { d->small_tiles = small; }
    ~SmallTiles() { d->small_tiles = was; }
};

}  // namespace xq

// kernels (each header opens namespace xq itself)
#include "xq_l0.hip.h"
#include "xq_td.hip.h"
#include "xq_tail.hip.h"
#include "xq_apply.hip.h"
#include "xq_refine.hip.h"
#include "xq_nstep.hip.h"
#include "xq_stage.hip.h"
#include "xq_legal.hip.h"

namespace xq {

// ---------------------------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------------------------
static inline int vec_ok(const void* p, long long ld) { return (((uintptr_t)p) % 16 == 0) && (ld % 4 == 0); }

// tile choice: 128x128 when that grid already fills the chip twice over, else 64x64 (4x the blocks)
template <int AL, int BL, int EPI, int DT = DT_F32>
static int launch_gemm(xq_dqn* d, GemmArgs g, int splits, const char* name, int* used_splits = nullptr, bool force_small = false) {
    if (used_splits) *used_splits = 0;
    if (g.M <= 0 || g.N <= 0 || g.K <= 0) return fail(XQ_ERR_INVALID_ARGUMENT, "empty GEMM %s (%d x %d x %d)", name, g.M, g.N, g.K);
    g.a_vec = vec_ok(g.A, g.lda);
    g.b_vec = vec_ok(g.B, g.ldb);
    if (splits < 1) splits = 1;
    g.k_chunk = round_up((g.K + splits - 1) / splits, GBK);
    splits = (g.K + g.k_chunk - 1) / g.k_chunk;
    if (splits < 1) splits = 1;
    const int groups = g.grouped > 1 ? g.grouped : 1;
    const long long t128 = (long long)((g.M + 127) / 128) * ((g.N + 127) / 128) * (g.grouped ? groups : splits);
    const bool big = (!force_small && !d->small_tiles && t128 >= 512);
    const double kk = DT == DT_BF16 ? 2.0 * g.K : (double)g.K;       // bf16: K counts pairs
    if (d->tail_open) {                  // fused tail launch (td_tail_kernel): the blocks join the open grid instead of launching
        TailArgs& T = *d->tail;
        const bool is_delta = AL == L_KCONTIG && BL == L_MCONTIG && EPI == EPI_DELTA, is_grad = AL == L_MCONTIG && BL == L_MCONTIG && EPI == EPI_STORE;
        if (DT != DT_F32 || big || g.grouped || !(is_delta || is_grad) || (is_delta && (T.n_delta || splits != 1)) || (is_grad && T.n_grad))
            return fail(XQ_ERR_RUNTIME, "GEMM %s cannot join the fused tail launch", name);
        const int gx = (g.M + 63) / 64, gy = (g.N + 63) / 64;
        if (is_delta) { T.delta = g; T.delta_gx = gx; T.n_delta = gx * gy; }
        else { T.grad = g; T.grad_gx = gx; T.grad_gy = gy; T.n_grad = gx * gy * splits; }
        d->tail_flops += 2.0 * g.M * g.N * kk;
        d->tail_bytes += 4.0 * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N);
        d->tail_lds = std::max(d->tail_lds, 2 * (size_t)g_tile_floats(64) * sizeof(float));
        if (used_splits) *used_splits = splits;
        return XQ_OK;
    }
    ProfScope ps(d, name, 2.0 * g.M * g.N * kk, 4.0 * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N));
    if (g.grouped) {
        if (splits != 1) return fail(XQ_ERR_INVALID_ARGUMENT, "grouped GEMM cannot be split-K");
        if (groups > 3) return fail(XQ_ERR_INVALID_ARGUMENT, "at most 3 grouped products");
        for (int k = 0; k + 1 < groups; ++k) {
            g.b_vec = g.b_vec && vec_ok(g.Bx[k], g.ldb);
            g.a_vec = g.a_vec && vec_ok(g.Ax[k], g.lda);
        }
        ps.flops *= groups; ps.bytes *= groups;
    }
    const int gz = g.grouped ? groups : splits;
    if (big) {
        dim3 grid((g.M + 127) / 128, (g.N + 127) / 128, gz);
        hipLaunchKernelGGL((gemm_f32_kernel<AL, BL, EPI, 2, 2, DT>), grid, dim3(256), 0, d->cur, g);
    } else {
        dim3 grid((g.M + 63) / 64, (g.N + 63) / 64, gz);
        hipLaunchKernelGGL((gemm_f32_kernel<AL, BL, EPI, 1, 1, DT>), grid, dim3(256), 0, d->cur, g);
    }
    XQ_HIP(hipGetLastError());
    if (used_splits) *used_splits = splits;
    return XQ_OK;
}

// A kernel's dynamic-LDS limit raised to `bytes` the first time it is asked for, per kernel address (every template instance has its own)
static int ensure_max_dynamic_lds(const void* kernel, int bytes) {
    static std::mutex m;
    static std::unordered_map<const void*, int> granted;
    std::lock_guard<std::mutex> lock(m);
    int& have = granted[kernel];
    if (have >= bytes) return XQ_OK;
    XQ_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    have = bytes;
    return XQ_OK;
}
template <class F> static int ensure_max_dynamic_lds(F* kernel, int bytes) { return ensure_max_dynamic_lds(reinterpret_cast<const void*>(kernel), bytes); }

// gemm_dma_kernel (xq_gemm_dma.hip.h): (128 TI) x (64 TJ) tiles, up to 144 KB of dynamic LDS
template <int DT, int AL, int BL, int EPI, int TI, int TJ>
static int launch_dma_gemm(xq_dqn* d, const Bf16GemmArgs& g, int gz, const char* name) {
    constexpr int lds = bg_lds_bytes(TI, TJ);
    XQ_TRY(ensure_max_dynamic_lds(gemm_dma_kernel<DT, AL, BL, EPI, TI, TJ>, lds));
    const int groups = g.groups > 1 ? g.groups : 1;
    const double es = DT == DT_F32 ? 4.0 : 2.0;
    ProfScope ps(d, name, 2.0 * g.M * g.N * (double)g.K * groups, es * groups * ((double)g.M * g.K + (double)g.N * g.K + 2.0 * g.M * g.N));
    hipLaunchKernelGGL((gemm_dma_kernel<DT, AL, BL, EPI, TI, TJ>), dim3(g.M / (128 * TI), g.N / (64 * TJ), gz), dim3(512), lds, d->cur, g);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}
template <int AL, int BL, int EPI>
static int launch_bf16_gemm(xq_dqn* d, const Bf16GemmArgs& g, int gz, const char* name) {
    return launch_dma_gemm<DT_BF16, AL, BL, EPI, 2, 2>(d, g, gz, name);
}

// The ensure_* functions: the size arithmetic of a family of workspaces.  Every buffer reserves on its own (DevBuf::reserve: free when
// it is large enough), so a growth that fails part-way leaves nothing to repair — the next call grows what is still too small.
// A buffer whose padding is read gets its zeros, on stream s, when it is new.
template <class T> static int reserve_zeroed(DevBuf<T>& b, size_t count, hipStream_t s) {
    bool grew = false;
    XQ_TRY(b.reserve(count, &grew));
    if (grew) XQ_HIP(hipMemsetAsync(b, 0, count * sizeof(T), s));
    return XQ_OK;
}

static int ensure_capacity(xq_dqn* d, int n) {
    const size_t cap = (size_t)n;
    int maxh = 0;
    for (int l = 0; l + 1 < d->nl; ++l) maxh = std::max(maxh, d->L[l + 1]);
    for (int l = 0; l + 1 < d->nl; ++l) {
        XQ_TRY(d->acts[l].reserve(cap * d->L[l + 1]));
        XQ_TRY(d->deltas[l].reserve(cap * d->L[l + 1]));
    }
    // rows padded to a multiple of 128 (whole-tile reads of the persistent GEMM)
    for (auto& t : d->tacts) XQ_TRY(reserve_zeroed(t, (size_t)round_up(n, 128) * (size_t)maxh, d->stream));
    const int ntn = (d->nout() + 63) / 64;             // column-max partials: 2 per 64- or 128-row tile
    XQ_TRY(d->q90.reserve(cap * 96));
    // (partials: the sample dimension padded to whole blocks of screen_top2_kernel, which stores every column of its panels)
    XQ_TRY(d->partial.reserve((size_t)round_up(n, 512) * (size_t)ntn * 2));
    for (DevBuf<float>* b : {&d->qsa, &d->yv, &d->lossv, &d->dsc}) XQ_TRY(b->reserve(cap));
    XQ_TRY(d->act_mb.reserve(cap));
    XQ_TRY(d->zmax.reserve(cap * kReduceParts));
    XQ_TRY(d->zidx.reserve(cap * kReduceParts));
    return d->gboards.reserve(cap * kBoardWords);
}

// the extra buffers of the build-defined modes, allocated on first use: bf16 bits of every activation buffer (bf16 Q-net), the
// third forward chain and the arg-max partials (Double DQN)
static int ensure_ext_capacity(xq_dqn* d, int n, bool want_double) {
    int maxh = 0;
    for (int l = 0; l + 1 < d->nl; ++l) maxh = std::max(maxh, d->L[l + 1]);
    const size_t rows = (size_t)round_up(n, 512);      // whole-tile reads of the persistent GEMM (128) / whole panels of screen_top2_kernel (512)
    if (d->bf16()) {
        for (int l = 0; l + 1 < d->nl; ++l) XQ_TRY(d->acts_bf[l].reserve(rows * d->L[l + 1]));
        for (int i = 0; i < 2; ++i) {
            XQ_TRY(reserve_zeroed(d->tacts_bf[i], rows * (size_t)maxh, d->stream));
            XQ_TRY(reserve_zeroed(d->t2acts_bf[i], rows * (size_t)maxh, d->stream));
        }
    }
    if (d->bf16_bwd())
        for (int l = 0; l + 1 < d->nl; ++l) XQ_TRY(d->deltas_bf[l].reserve(rows * d->L[l + 1]));
    if (want_double) {
        for (auto& t : d->t2acts) XQ_TRY(reserve_zeroed(t, rows * (size_t)maxh, d->stream));
        const int ntn = (d->nout() + 63) / 64;
        XQ_TRY(d->partial_idx.reserve(rows * (size_t)ntn * 2));
    }
    return XQ_OK;
}

static SlotSrc explicit_slots(const int32_t* slots) {
    SlotSrc s; memset(&s, 0, sizeof s); s.slots = slots; return s;
}

// totals of the per-block candidate counters: the carry plus a host copy `h` of the array ...
void Screen::totals_of(const unsigned long long* h, unsigned long long sums[2]) const {
    sums[0] = carry[0]; sums[1] = carry[1];
    for (int i = 0; i < stat_blocks; ++i) { sums[0] += h[2 * i]; sums[1] += h[2 * i + 1]; }
}
// ... or of the array as it stands (synchronises the device)
int Screen::totals(unsigned long long sums[2]) const {
    std::vector<unsigned long long> h((size_t)2 * stat_blocks);
    if (stat_blocks) {
        XQ_HIP(hipDeviceSynchronize());
        XQ_HIP(hipMemcpy(h.data(), stats, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    totals_of(h.data(), sums);
    return XQ_OK;
}
// buffers of the screened maximum (xq_dqn_set_qmax_mode), allocated on first use (params, acts: for the XQ_DEBUG_PTRS print alone)
int Screen::reserve(int NO, int Hl, int n, const void* params, const void* acts) {
    const size_t wrows = (size_t)round_up(NO, 128);
    bool grew = false;
    XQ_TRY(wb.reserve(wrows * Hl, &grew));
    if (grew) {
        XQ_HIP(hipMemset(wb, 0, wrows * Hl * sizeof(uint16_t)));
        static_net = -1;
    }
    grew = false;
    XQ_TRY(wmax.reserve(6, &grew));
    if (grew) XQ_HIP(hipMemset(wmax, 0, 6 * sizeof(unsigned)));
    XQ_TRY(guard_ev.create(hipEventDisableTiming));
    // sample dimension padded to whole blocks of screen_top2_kernel (512): it stores every column of its panels unconditionally
    const size_t rows = (size_t)round_up(n, 512), G = (size_t)4 * ((NO + 127) / 128);
    grew = false;
    XQ_TRY(ab.reserve(rows * Hl, &grew));
    if (grew) XQ_HIP(hipMemset(ab, 0, rows * Hl * sizeof(uint16_t)));
    XQ_TRY(p1.reserve(G * rows, &grew));
    XQ_TRY(p2.reserve(G * rows, &grew));
    XQ_TRY(R.reserve((size_t)((NO + 63) / 64) * rows, &grew));       // at most one range per 64-row chunk
    XQ_TRY(na.reserve(rows, &grew));
    if (grew)
        if (const char* e = getenv("XQ_DEBUG_PTRS")) if (e[0] == '1')
            fprintf(stderr, "[xq] screening buffers: P1 %p P2 %p R %p ab %p na %p params %p acts %p\n", (void*)p1.p, (void*)p2.p,
                    (void*)R.p, (void*)ab.p, (void*)na.p, params, acts);
    // candidate counters: one pair per refine block (32 samples); the totals of the array it replaces are carried on the host.
    // stat_blocks is the capacity of the pair (array + pinned copy): 0 while it is being replaced, so that a failure in between
    // leaves totals that totals() still gets right and a pair that the next call allocates again
    const int blocks = (int)(rows / kRefineSamples);
    if (blocks > stat_blocks) {
        if (stat_blocks) {
            unsigned long long sums[2];
            XQ_TRY(totals(sums));
            carry[0] = sums[0]; carry[1] = sums[1];
            guard_pending = false;
        }
        stat_blocks = 0;
        XQ_TRY(stats.reserve((size_t)2 * blocks));
        XQ_HIP(hipMemset(stats, 0, stats.n * sizeof(unsigned long long)));
        XQ_TRY(guard_host.reserve((size_t)2 * blocks));
        memset(guard_host, 0, guard_host.n * sizeof(unsigned long long));
        stat_blocks = blocks;
    }
    return XQ_OK;
}

// One forward chain of a launch group: a_1 .. a_{nl-1} of `net` for n packed boards; outs[l] receives a_{l+1} in fp32 (may be
// nullptr per chain in bf16 mode when only the next layer reads it), outs_bf[l] its bf16 bits (bf16 Q-net only).
// Up to three chains run in the same launches: one gather grid with blockIdx.y = chain, grouped GEMMs with blockIdx.z = chain.
struct ChainJob {
    int net;
    const uint32_t* boards;
    float* const* outs;
    uint16_t* const* outs_bf;
    uint32_t* gathered;
    uint16_t* last_bf;          // fp32 net: != nullptr => bf16 copy of the chain's LAST hidden activations (screening operand)
    bool last_bf_frag;          //   ... written in MFMA B-fragment order (scr_afrag_index) for screen_top2_kernel
    float* head_slabs;          // fp32 net, one chain, >= 2 hidden layers: != nullptr => the select head's k-slabs [hlast / 64][n][96] come
                                //   out of the last hidden product (EPI_HEAD); the last activations are stored only if outs[nl-2] != nullptr
    int sel_keep;               // fp32 net, one chain: 1 = layer 0 through l0_select_kernel (sums kept in sel_state->z1 for the next ply),
                                //   2 = ... and derived from the sums kept last time
};
// A chain's views into a family of workspaces: a_{l+1} in buffer l % period of `fp` (nullptr unless `fp32`) and of `bits`
static void chain_views(const xq_dqn* d, const DevBuf<float>* fp, const DevBuf<uint16_t>* bits, int period, bool fp32, float** outs, uint16_t** outs_bf) {
    for (int l = 0; l + 1 < d->nl; ++l) { outs[l] = fp32 ? fp[l % period].p : nullptr; outs_bf[l] = bits[l % period]; }
}
// Chain k's operands in a grouped argument block (GemmArgs, Bf16GemmArgs): group 0 in the plain fields, group k in slot k - 1 of the *x arrays
template <class G, class T>
static void set_group(G& g, int k, const T* A, const T* B, float* C, const float* bias, uint16_t* Cb) {
    if (k == 0) { g.A = A; g.B = B; g.C = C; g.bias = bias; g.Cb = Cb; }
    else { g.Ax[k - 1] = A; g.Bx[k - 1] = B; g.Cx[k - 1] = C; g.biasx[k - 1] = bias; g.Cbx[k - 1] = Cb; }
}

// Layer 0 of one fp32 chain through l0_select_kernel: the sums are kept for the next ply, or derived from those kept last time
static int l0_select_forward(xq_dqn* d, const ChainJob& job, int n) {
    const int H = d->L[1];
    ProfScope ps(d, "l0_forward_gather", 2.0 * n * 32 * H, (double)n * (96 + (job.sel_keep == 2 ? 4.0 : 32.0) * H * 4 + H * 12), true);
    xq_dqn::SelKeep& K = d->sel_keep[d->cur == d->stream ? 0 : 1];
    hipExtLaunchKernelGGL(l0_select_kernel, dim3((n + 3) / 4), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, job.boards, K.prev_boards.p, d->w0t(job.net),
                       d->bl(job.net, 0), K.z1.p, job.outs[0], n, H, job.sel_keep == 2 ? 1 : 0);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}
// Layer 0 of up to three chains in one gather grid (blockIdx.y = chain), the s' chain derived and the screening shadow riding where they can
static int l0_forward(xq_dqn* d, const ChainJob* jobs, int njobs, SlotSrc src, int n, const ShadowJob* shadow) {
    const int H = d->L[1];
    const bool bf = d->bf16();
    L0Jobs J; memset(&J, 0, sizeof J);
    J.njobs = njobs;
    for (int k = 0; k < njobs; ++k) {
        J.boards[k] = jobs[k].boards; J.W0T[k] = d->w0t(jobs[k].net); J.b0[k] = d->bl(jobs[k].net, 0);
        J.out[k] = jobs[k].outs ? jobs[k].outs[0] : nullptr; J.gathered[k] = jobs[k].gathered;
        if (bf) { J.W0T_bf[k] = d->wl_bf(jobs[k].net, 0); J.out_bf[k] = jobs[k].outs_bf[0]; }
        else if (d->nl == 2) { J.out_bf[k] = jobs[k].last_bf; if (jobs[k].last_bf && jobs[k].last_bf_frag) J.out_bf_frag = 1; }
    }
    // online TD rule on an fp32 net: the s' chain (job 1, same net, same slots) is derived inside job 0's waves
    // (bf16 net: in the 16-byte gather path only; Double DQN's third chain — the target net — is gathered as before)
    const bool wide_bf = bf && (H & 7) == 0 && ((H >= 512 && (H & 511) == 0) || (H >= 64 && 512 % H == 0));
    const bool derive = d->l0_derive && njobs >= 2 && jobs[0].net == jobs[1].net && jobs[1].gathered == nullptr &&
                        (bf ? wide_bf : (njobs == 2 && (H & 3) == 0));
    J.derive_next = derive ? 1 : 0;
    J.nrows = njobs - (derive ? 1 : 0);
    // the screening shadow of the output-layer weights rides in the same grid (one more row of blocks) when the grid is wide
    // enough for it; a launch of its own otherwise
    const bool ride = shadow && shadow->nblocks <= (n + 3) / 4;
    if (ride) J.shadow = *shadow;
    else if (shadow) {
        hipLaunchKernelGGL(screen_shadow_kernel, dim3(shadow->nblocks), dim3(256), 0, d->cur, *shadow);
        XQ_HIP(hipGetLastError());
    }
    ProfScope ps(d, "l0_forward_gather", 2.0 * njobs * n * 32 * H, (double)njobs * n * (48 + 32.0 * H * (bf ? 2 : 4) + H * 4), true);
    // (grid rows: the job rows that are really gathered, then the shadow row; the kernel tests blockIdx.y == J.nrows for it)
    if (bf) hipExtLaunchKernelGGL(l0_forward_kernel<true>, dim3((n + 3) / 4, J.nrows), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, J, src, n, H);
    else hipExtLaunchKernelGGL(l0_forward_kernel<false>, dim3((n + 3) / 4, J.nrows + (ride ? 1 : 0)), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, J, src, n, H);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// The hidden products a_{l+1} = tanh(W_l a_l + b_l) of the chains (the groups of one launch); hidden_forward picks the first whose test holds.
// bf16 net, whole 256 x 128 tiles: the bf16 loop of its own (xq_gemm_dma.hip.h)
static bool hidden_bf16_dma_shape(const xq_dqn* d, int l, int n) { return (n % kBgBM) == 0 && (d->L[l + 1] % kBgBN) == 0 && (d->L[l] % kBgBK) == 0; }
static int hidden_bf16_dma(xq_dqn* d, const ChainJob* jobs, int njobs, int l, int n) {
    Bf16GemmArgs b; memset(&b, 0, sizeof b);
    b.M = n; b.N = d->L[l + 1]; b.K = d->L[l]; b.lda = b.ldb = d->L[l]; b.k_chunk = b.K;
    b.ldc = b.ldcb = d->L[l + 1]; b.groups = njobs;
    for (int k = 0; k < njobs; ++k) {
        set_group(b, k, jobs[k].outs_bf[l - 1], d->wl_bf(jobs[k].net, l), jobs[k].outs ? jobs[k].outs[l] : nullptr, d->bl(jobs[k].net, l), jobs[k].outs_bf[l]);
        // the chain's last activations in B-fragment order when only screen_top2_kernel reads them (bf16 net: max / arg-max pass)
        if (l == d->nl - 2 && jobs[k].last_bf_frag) b.cb_frag_mask |= 1 << k;
    }
    return launch_bf16_gemm<L_KCONTIG, L_KCONTIG, BG_TANH>(d, b, njobs, "gemm_hidden_fwd");
}
// M, N, K (kdiv = 2: bf16 pairs), the leading dimensions and the group count of layer l's product on the tile kernels
static GemmArgs hidden_tile_shape(const xq_dqn* d, int njobs, int l, int n, int kdiv) {
    GemmArgs g; memset(&g, 0, sizeof g);
    g.M = n; g.N = d->L[l + 1]; g.K = d->L[l] / kdiv;
    g.grouped = njobs > 1 ? njobs : 0;
    g.lda = g.ldb = g.K; g.ldc = g.ldcb = d->L[l + 1];
    return g;
}
// bf16 net, any other shape: the tile kernel on bf16 pairs
static int hidden_bf16_tile(xq_dqn* d, const ChainJob* jobs, int njobs, int l, int n) {
    if (d->L[l] & 1) return fail(XQ_ERR_INVALID_ARGUMENT, "bf16 Q-net needs even layer widths (layer %d has %d)", l, d->L[l]);
    GemmArgs g = hidden_tile_shape(d, njobs, l, n, 2);
    for (int k = 0; k < njobs; ++k)
        set_group(g, k, reinterpret_cast<const float*>(jobs[k].outs_bf[l - 1]), reinterpret_cast<const float*>(d->wl_bf(jobs[k].net, l)),
                  jobs[k].outs ? jobs[k].outs[l] : nullptr, d->bl(jobs[k].net, l), jobs[k].outs_bf[l]);
    return launch_gemm<L_KCONTIG, L_KCONTIG, EPI_BIAS_TANH, DT_BF16>(d, g, 1, "gemm_hidden_fwd");
}
// fp32 net, the last hidden product of one chain that asks for it: the select head rides (EPI_HEAD; its k-slabs instead of a_last)
static int hidden_f32_head(xq_dqn* d, const ChainJob& job, int l, int n) {
    GemmArgs g = hidden_tile_shape(d, 1, l, n, 1);
    if ((n & 63) || (g.N & 63) || (g.K & 31) || d->nout() < 128) return fail(XQ_ERR_RUNTIME, "select head cannot ride on this hidden product");
    set_group(g, 0, job.outs[l - 1], d->wl(job.net, l), job.outs[l], d->bl(job.net, l), nullptr);
    g.a_vec = vec_ok(g.A, g.lda); g.b_vec = vec_ok(g.B, g.ldb); g.k_chunk = g.K;
    g.head_W = d->wl(job.net, d->nl - 1); g.head_ldw = g.N;
    g.head_slabs = job.head_slabs; g.head_slab_stride = (long long)n * 96; g.head_ld = 96;
    if (!g.a_vec || !g.b_vec || !vec_ok(g.head_W, g.head_ldw)) return fail(XQ_ERR_RUNTIME, "select head: unaligned operand");
    ProfScope ps(d, "gemm_hidden_fwd", 2.0 * n * g.N * (g.K + 96.0), 4.0 * ((double)n * g.K + (double)g.N * g.K + (double)(g.N / 64) * n * 96), true);
    hipExtLaunchKernelGGL((gemm_f32_kernel<L_KCONTIG, L_KCONTIG, EPI_HEAD, 1, 1>), dim3(n / 64, g.N / 64, 1), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, g);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}
// fp32 net: the operands of the chains, for the walk and the tile kernel alike; *aligned: every A and B takes 16-byte loads
static GemmArgs hidden_f32_args(const xq_dqn* d, const ChainJob* jobs, int njobs, int l, int n, bool* aligned) {
    GemmArgs g = hidden_tile_shape(d, njobs, l, n, 1);
    *aligned = true;
    for (int k = 0; k < njobs; ++k) {
        uint16_t* cb = (l == d->nl - 2) ? jobs[k].last_bf : nullptr;
        if (cb && jobs[k].last_bf_frag) g.cb_frag = 1;
        set_group(g, k, jobs[k].outs[l - 1], d->wl(jobs[k].net, l), jobs[k].outs[l], d->bl(jobs[k].net, l), cb);
        *aligned = *aligned && vec_ok(jobs[k].outs[l - 1], g.lda) && vec_ok(d->wl(jobs[k].net, l), g.ldb);
    }
    return g;
}
// fp32 net, whole 128-row x 128-column tiles, not the select chain: the persistent walk (gemm_fwd_persistent_kernel; same bits as the
// tile kernel).  8192 x 512 x 512 x 2 chains: 90 -> 76 us (128 x 128 tiles, 2 blocks per CU walk 512 tiles); 8192 x 256 x 256 x 2:
// 27.5 -> 26.3 us (64 x 128 tiles) — tools/f32_fwd_probe.hip.  stop_ev: the event the trainer's select chain waits for rides on this
// kernel's own completion signal when it is the last of the chains on the handle's stream (no marker packet: ~1.5 us less than a record,
// tools/sync_probe.hip variant 5) — taken = cleared; a launch that is being timed carries the profiler's events and leaves it to the caller
static int hidden_f32_walk(xq_dqn* d, GemmArgs g, int l, hipEvent_t* stop_ev) {
    const int n = g.M, groups = g.grouped > 1 ? g.grouped : 1;
    const bool big = (n / 128) * (g.N / 128) * groups >= 512;              // 128 x 128 tiles, else 64 x 128
    const int tiles_m = big ? n / 128 : n / 64, total = tiles_m * (g.N / 128) * groups;
    g.k_chunk = g.K; g.a_vec = g.b_vec = 1;
    ProfScope ps(d, "gemm_hidden_fwd", 2.0 * n * (double)g.N * g.K * groups, 4.0 * groups * ((double)n * g.K + (double)g.N * g.K + (double)n * g.N), true);
    hipEvent_t stop = ps.stop();
    if (!stop && stop_ev && l == d->nl - 2 && d->cur == d->stream) { stop = *stop_ev; *stop_ev = nullptr; }
    hipExtLaunchKernelGGL(big ? gemm_fwd_persistent_kernel<2, 2, 2> : gemm_fwd_persistent_kernel<1, 2, 2>, dim3(std::min(total, 2 * d->ncu)), dim3(256), 0,
                          d->cur, ps.start(), stop, 0, g, tiles_m, g.N / 128, total);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}
static int hidden_forward(xq_dqn* d, const ChainJob* jobs, int njobs, int l, int n, hipEvent_t* stop_ev) {
    if (d->bf16()) return hidden_bf16_dma_shape(d, l, n) ? hidden_bf16_dma(d, jobs, njobs, l, n) : hidden_bf16_tile(d, jobs, njobs, l, n);
    if (l == d->nl - 2 && njobs == 1 && jobs[0].head_slabs) return hidden_f32_head(d, jobs[0], l, n);
    bool aligned = true;
    const GemmArgs g = hidden_f32_args(d, jobs, njobs, l, n, &aligned);
    if (aligned && !d->small_tiles && !d->tail_open && (n % 128) == 0 && (g.N % 128) == 0 && (g.K % GBK) == 0) return hidden_f32_walk(d, g, l, stop_ev);
    return launch_gemm<L_KCONTIG, L_KCONTIG, EPI_BIAS_TANH>(d, g, 1, "gemm_hidden_fwd");       // any other shape, and the select chain: the tile kernel
}

// The forward chains of a launch group.  stop_ev (optional): see hidden_f32_walk — still set on return when no product could take it
static int chain_boards(xq_dqn* d, const ChainJob* jobs, int njobs, SlotSrc src, int n, const ShadowJob* shadow = nullptr, hipEvent_t* stop_ev = nullptr) {
    if (d->L[0] != kStateSize) return fail(XQ_ERR_INVALID_ARGUMENT, "board input needs layer_sizes[0] == 1260 (got %d)", d->L[0]);
    if (njobs < 1 || njobs > kMaxChains) return fail(XQ_ERR_INVALID_ARGUMENT, "1..3 forward chains per launch group");
    if (njobs == 1 && jobs[0].sel_keep && !d->bf16() && !shadow && !src.implicit && !src.slots) XQ_TRY(l0_select_forward(d, jobs[0], n));
    else XQ_TRY(l0_forward(d, jobs, njobs, src, n, shadow));
    for (int l = 1; l + 1 < d->nl; ++l) XQ_TRY(hidden_forward(d, jobs, njobs, l, n, stop_ev));
    return XQ_OK;
}

// k-slabs of the select head for the stream the launches go to: the select chain may run on its own stream beside a TD step or a
// query on the handle's, so each of the two has its own
static int head_slabs(xq_dqn* d, size_t floats, float** slab) {
    DevBuf<float>& b = d->qh_slabs[d->cur == d->stream ? 0 : 1];
    XQ_TRY(b.reserve(floats));
    *slab = b;
    return XQ_OK;
}
// q[m][0..n_out) = tanh(the ordered sum of the head's k-slabs + bias) (q_head_finish_kernel); name != nullptr: bracketed under it
static int q_head_finish(xq_dqn* d, const float* slab, long long slab_stride, int nslabs, int n, int n_out, int nc, const float* bias, float* q, int ldq,
                         const char* name = nullptr) {
    ProfScope ps(d, name, (double)n * n_out * nslabs, 4.0 * n * n_out * (nslabs + 1));
    hipLaunchKernelGGL(q_head_finish_kernel, dim3((unsigned)(((long long)n * n_out + 255) / 256)), dim3(256), 0, d->cur, slab, slab_stride, nslabs, n, n_out, nc,
                       bias, q, ldq);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// Q head on the first n_out outputs: q[m][0..n_out) = tanh(W_out[0:n_out] a_last + b_out); a_last_bf != nullptr: bf16 operands
// (weights from the shadow), fp32 result (the output layer is never rounded)
static int q_head(xq_dqn* d, int net, const float* a_last, int n, int n_out, float* q, int ldq, const char* name,
                  const uint16_t* a_last_bf = nullptr) {
    GemmArgs g; memset(&g, 0, sizeof g);
    g.M = n; g.N = n_out; g.bias = d->bl(net, d->nl - 1);
    if (a_last_bf) {
        g.K = d->hlast() / 2;
        g.A = reinterpret_cast<const float*>(a_last_bf); g.lda = d->hlast() / 2;
        g.B = reinterpret_cast<const float*>(d->wl_bf(net, d->nl - 1)); g.ldb = d->hlast() / 2;
        g.C = q; g.ldc = ldq;
        return launch_gemm<L_KCONTIG, L_KCONTIG, EPI_BIAS_TANH, DT_BF16>(d, g, 1, name);
    }
    g.K = d->hlast();
    g.A = a_last; g.lda = d->hlast();
    g.B = d->wl(net, d->nl - 1); g.ldb = d->hlast();
    g.libm_tanh = 1;                     // the output layer's tanh stays libm's (as in q_head_finish_kernel / the env kernel / the TD kernels)
    // The select head (selectAction reads q[action.to] only, dqn.cpp:47): 8192 x 96 x K is two column tiles of 64 — 256 blocks, one per
    // CU, each walking all K / 32 k-tiles behind one another with nothing to hide the load latency behind (20 us at K = 256, 32 us at
    // K = 512 for 0.4 / 0.8 GFLOP).  Four k-slabs per tile put four blocks on every CU; a one-thread-per-output kernel adds the slabs in a
    // fixed order, the bias and the tanh.  fp32 nets, large batches (the small ones are not latency-bound per CU to begin with).
    // The slabs are 64 columns of the last hidden layer each — what the fused form (EPI_HEAD in chain_boards, dqn_q90_boards) produces
    // per column tile, so both forms give the same bits.
    if (n_out <= 96 && n >= 2048 && (g.K % 128) == 0) {
        const int nc = round_up(n_out, 4);
        const int nslabs = g.K / 64;
        const size_t need = (size_t)nslabs * n * nc;
        float* slab = nullptr;
        XQ_TRY(head_slabs(d, need, &slab));
        g.C = slab; g.ldc = nc; g.slab_stride = (long long)n * nc;
        XQ_TRY((launch_gemm<L_KCONTIG, L_KCONTIG, EPI_STORE>(d, g, nslabs, name, nullptr, true)));
        return q_head_finish(d, slab, g.slab_stride, nslabs, n, n_out, nc, g.bias, q, ldq);
    }
    g.C = q; g.ldc = ldq;
    return launch_gemm<L_KCONTIG, L_KCONTIG, EPI_BIAS_TANH>(d, g, 1, name);
}

static int ensure_select_capacity(xq_dqn* d, int n) {
    for (int l = 0; l + 1 < d->nl; ++l) XQ_TRY(d->sel_acts[l].reserve((size_t)n * d->L[l + 1]));
    XQ_TRY(d->sel_q90.reserve((size_t)n * 96));
    for (int l = 0; d->bf16() && l + 1 < d->nl; ++l) XQ_TRY(d->sel_acts_bf[l].reserve((size_t)round_up(n, 128) * d->L[l + 1]));
    return XQ_OK;
}

// Q(s)[0..95] of n packed boards on the online net.  `on` != nullptr queues the chain on that stream with its own
// workspace and 64x64 tiles, so it can run concurrently with a TD step queued on the handle's stream.
int dqn_q90_boards(xq_dqn* d, const uint32_t* boards_dev, int n, float** q90_dev, int* q_stride, hipStream_t on, QSource* qs) {
    if (d->nout() < 96) return fail(XQ_ERR_INVALID_ARGUMENT, "self-play select needs >= 96 outputs");
    if (qs) memset(qs, 0, sizeof *qs);
    float* outs[XQ_MAX_LAYERS];
    uint16_t* outs_bf[XQ_MAX_LAYERS] = {nullptr};
    const bool bf = d->bf16();
    if (on) XQ_TRY(ensure_select_capacity(d, n));
    else {
        XQ_TRY(ensure_capacity(d, n));
        XQ_TRY(ensure_ext_capacity(d, n, false));
    }
    chain_views(d, on ? d->sel_acts : d->acts, on ? d->sel_acts_bf : d->acts_bf, XQ_MAX_LAYERS, !bf, outs, outs_bf);
    float* q = on ? d->sel_q90 : d->q90;
    OnStream on_stream(d, on ? on : d->cur);          // restored on every way out, like the tile choice
    SmallTiles small(d, on != nullptr);
    ChainJob job{XQ_NET_ONLINE, boards_dev, outs, outs_bf, nullptr};
    // layer-0 sums kept from ply to ply (xq_dqn_set_l0_derive) — when that pays: keeping costs 16 MB of stores per call, deriving saves
    // ~20 row reads per board, so it is used from the second call of an update period on and, once a period had several calls, from
    // its first (one ply per update, the headline: never; bench --config 4, four plies: 0.976 -> 0.964 ms)
    xq_dqn::SelKeep& K = d->sel_keep[on ? 1 : 0];
    K.calls += 1;
    const bool kept = d->l0_derive && !bf && (d->L[1] & 3) == 0 && (K.pays || K.calls >= 2);
    if (kept) {
        if ((size_t)n * d->L[1] > K.z1.n) K.valid = false;          // new buffers keep nothing (nor does a growth that fails)
        job.sel_keep = (K.valid && K.boards == boards_dev && K.n == n) ? 2 : 1;
        K.valid = false;                   // true again once every launch of this call has been queued
        XQ_TRY(K.z1.reserve((size_t)n * d->L[1]));
        XQ_TRY(K.prev_boards.reserve((size_t)n * kBoardWords));
    }
    // fp32 net with >= 2 hidden layers, whole 64 x 64 tiles, the batch sizes q_head splits into k-slabs: the head rides on the last hidden
    // product (same slabs, same bits) — its operand never goes to HBM and back (2 x 17 MB at 8192 x 512), one launch fewer per ply
    const int Hl = d->hlast();
    const bool ride = !bf && d->nl >= 3 && n >= 2048 && (n & 63) == 0 && (Hl % 128) == 0 && (d->L[d->nl - 2] & 31) == 0 && d->nout() >= 128 &&
                      vec_ok(d->wl(XQ_NET_ONLINE, d->nl - 1), Hl) && vec_ok(d->wl(XQ_NET_ONLINE, d->nl - 2), d->L[d->nl - 2]);
    if (ride) {
        const int nslabs = Hl / 64;
        float* slab = nullptr;
        XQ_TRY(head_slabs(d, (size_t)nslabs * n * 96, &slab));
        job.head_slabs = slab;
        outs[d->nl - 2] = nullptr;                       // nobody else reads the select chain's last activations
        XQ_TRY(chain_boards(d, &job, 1, explicit_slots(nullptr), n));
        if (qs) {                                        // the env kernel finishes the values it needs itself
            qs->slabs = slab; qs->slab_stride = (long long)n * 96; qs->nslabs = nslabs; qs->bias = d->bl(XQ_NET_ONLINE, d->nl - 1);
            q = nullptr;
        } else XQ_TRY(q_head_finish(d, slab, (long long)n * 96, nslabs, n, 96, 96, d->bl(XQ_NET_ONLINE, d->nl - 1), q, 96, "gemm_q90_select"));
    } else {
        XQ_TRY(chain_boards(d, &job, 1, explicit_slots(nullptr), n));
        XQ_TRY(q_head(d, XQ_NET_ONLINE, outs[d->nl - 2], n, 96, q, 96, "gemm_q90_select", bf ? outs_bf[d->nl - 2] : nullptr));
    }
    if (kept) { K.valid = true; K.boards = boards_dev; K.n = n; }
    *q90_dev = q;
    *q_stride = 96;
    return XQ_OK;
}

// conditions under which dqn.cu:406-423 as written stays inside its buffers (last paragraph)
static int check_reference_topology(const xq_dqn* d) {
    for (int l = d->nl - 2; l >= 0; --l) {
        const int inputSize = d->L[l + 1], outputSize = d->L[l];
        if (d->L[l + 2] < inputSize || outputSize < d->L[l + 1] ||
            d->wo[l + 1] + (size_t)(inputSize - 1) * outputSize + (size_t)(d->L[l + 1] - 1) >= d->nw)
            return fail(XQ_ERR_UNDEFINED_UPSTREAM,
                        "bug-compatible backprop reads out of bounds upstream for this topology (layer %d)", l);
    }
    return XQ_OK;
}

// matrix-pipe form of the layer-0 gradient (xq_dqn_set_l0_grad_mode(1), xq_l0grad.hip.h): taken at these shapes
static bool l0_mfma_shape(const xq_dqn* d, int n) { return d->l0_mfma && (d->L[1] % 64) == 0 && n >= 256; }
static int l0_chunk_of(int n) { return n >= 16384 ? 2048 : 1024; }
static int ensure_l0_mfma(xq_dqn* d, int n) {
    const int H = d->L[1], chunk = l0_chunk_of(n), kpad = (n + chunk - 1) / chunk * chunk;
    XQ_TRY(reserve_zeroed(d->l0_planes, l0m_plane_elems(H, kpad), d->cur));     // (the slack behind the planes is read, never used)
    if (!d->l0_hot.p) {                          // once per handle: the process's table, copied as it stands
        const L0HotTable& t = l0_hot_table();
        if (!t.ok) return fail(XQ_ERR_RUNTIME, "hot-row table: the reachable rows do not fit %d groups of %d", kL0HotGroups, kL0HotGroupRows);
        XQ_TRY(d->l0_hot.reserve(sizeof(L0HotTable) / sizeof(uint16_t)));
        XQ_HIP(hipMemcpyAsync(d->l0_hot.p, &t, sizeof t, hipMemcpyHostToDevice, d->cur));
    }
    XQ_TRY(d->l0_cold_list.reserve(l0cold_elems(kpad)));
    XQ_TRY(d->l0_cold_cnt.reserve((size_t)kpad / 64));
    return reserve_zeroed(d->l0_sel, l0sel_elems(kpad), d->cur);
}

// hidden deltas l = nl-2 .. 0 from the output-side delta `dnext` ([n][ld_next], only the first k_nz columns can be
// non-zero).  reference mode: delta_l = (dnext[:, :L[l+1]] x View) * (1-a^2), View[i][idx] = Wflat[wo[l+1] + i*L[l] + idx];
// textbook: View[k][idx] = W_{l+1}[k][idx], k < L[l+2].
static bool grad_bf16_ok(const xq_dqn* d, int M, int N, int K);
static int hidden_deltas(xq_dqn* d, int n, const float* dnext, int ld_next, int k_nz, int mode, int l_start = -1, int l_stop = 0) {
    const float* up = dnext;
    int ld_up = ld_next, nz = k_nz;
    if (l_start < 0) l_start = d->nl - 2;
    for (int l = l_start; l >= l_stop; --l) {
        GemmArgs g; memset(&g, 0, sizeof g);
        g.M = n; g.N = d->L[l + 1];
        const int kfull = (mode == XQ_BACKPROP_REFERENCE) ? d->L[l + 1] : d->L[l + 2];
        g.K = std::min(kfull, nz);
        if (d->bf16_bwd() && up == d->deltas[l + 1] && (n % kBgBM) == 0 && (g.N % kBgBN) == 0 && (g.K % kBgBK) == 0) {
            // XQ_PRECISION_BF16_FULL: delta_l = (bf16(delta_{l+1}) . bf16 weight VIEW) (1 - a_l^2) on the bf16 loop — the view is the
            // same (base, leading dimension) trick as below, applied to the bf16 shadow, which keeps the element order of the master
            Bf16GemmArgs b; memset(&b, 0, sizeof b);
            b.M = n; b.N = g.N; b.K = g.K; b.k_chunk = b.K;
            b.A = d->deltas_bf[l + 1]; b.lda = ld_up;
            b.B = d->wl_bf(XQ_NET_ONLINE, l + 1); b.ldb = (mode == XQ_BACKPROP_REFERENCE) ? d->L[l] : d->L[l + 1];
            b.C = d->deltas[l]; b.ldc = d->L[l + 1];
            b.Cb = d->deltas_bf[l]; b.ldcb = d->L[l + 1];
            b.Hb = d->acts_bf[l]; b.ldh = d->L[l + 1];
            XQ_TRY((launch_bf16_gemm<L_KCONTIG, L_MCONTIG, BG_DELTA>(d, b, 1, "gemm_hidden_delta")));
            up = d->deltas[l]; ld_up = d->L[l + 1]; nz = d->L[l + 1];
            continue;
        }
        g.A = up; g.lda = ld_up;
        g.B = d->wrest(XQ_NET_ONLINE) + (d->wo[l + 1] - d->wo[1]);
        g.ldb = (mode == XQ_BACKPROP_REFERENCE) ? d->L[l] : d->L[l + 1];
        g.C = d->deltas[l]; g.ldc = d->L[l + 1];
        g.H = d->acts[l]; g.ldh = d->L[l + 1];
        if (l == 0 && l0_mfma_shape(d, n) && (n % l0_chunk_of(n)) == 0) {
            // delta_0's planes for the matrix-pipe layer-0 gradient straight from this product's epilogue (64 x 64 tiles; whole tiles
            // and whole chunks only: the planes' zero padding is then empty) — no split launch, no re-read of delta_0
            const long long t128 = (long long)((g.M + 127) / 128) * ((g.N + 127) / 128);
            if (d->small_tiles || t128 < 512) {
                XQ_TRY(ensure_l0_mfma(d, n));
                g.split_planes = d->l0_planes; g.split_ld = n; g.split_plane_stride = (long long)d->L[1] * n;
                d->l0_split_done = true;
            }
        }
        XQ_TRY((launch_gemm<L_KCONTIG, L_MCONTIG, EPI_DELTA>(d, g, 1, "gemm_hidden_delta")));
        if (d->bf16_bwd() && l >= 1) {
            // XQ_PRECISION_BF16_FULL off the whole tiles: this product leaves no bf16 copy of delta_l, and the products that read one (the
            // delta below, this layer's weight gradient) pick the bf16 loop by their OWN shapes — rounded here when one of them does
            const int k_below = std::min(mode == XQ_BACKPROP_REFERENCE ? d->L[l] : d->L[l + 1], d->L[l + 1]);
            const bool delta_below = (n % kBgBM) == 0 && (d->L[l] % kBgBN) == 0 && (k_below % kBgBK) == 0;
            if (delta_below || grad_bf16_ok(d, d->L[l + 1], d->L[l], n)) {
                hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(std::min((n * d->L[l + 1] + 255) / 256, 1024)), dim3(256), 0, d->cur, d->deltas[l].p,
                                   d->deltas_bf[l].p, (long long)n * d->L[l + 1]);
                XQ_HIP(hipGetLastError());
            }
        }
        up = d->deltas[l]; ld_up = d->L[l + 1]; nz = d->L[l + 1];
    }
    return XQ_OK;
}

// gradient GEMMs always use 64x64 tiles: more tiles => fewer k-splits => less slab traffic in the ordered reduction
static int pick_splits(int M, int N, int K) {
    const int tiles = ((M + 63) / 64) * ((N + 63) / 64);
    int s = (512 + tiles - 1) / tiles;
    s = std::min(s, std::max(1, K / 128));
    return std::max(1, std::min(s, 32));
}

// XQ_PRECISION_BF16_FULL: the hidden weight gradient on the bf16 loop when the shape allows (whole 256 x 128 tiles, whole 64-deep
// k-tiles per slab); the slab count then comes from the 256 x 128 tiling: one block per CU
static bool grad_bf16_ok(const xq_dqn* d, int M, int N, int K) {
    return d->bf16_bwd() && (M % kBgBM) == 0 && (N % kBgBN) == 0 && K >= kBgBK && (K % kBgBK) == 0;
}
static int grad_splits(const xq_dqn* d, int M, int N, int K) {
    if (!grad_bf16_ok(d, M, N, K)) return pick_splits(M, N, K);
    const int tiles = (M / kBgBM) * (N / kBgBN);
    int s = std::max(1, d->ncu / tiles);
    s = std::min(s, 16);                                    // (32 slabs = one block per CU: 0.717 ms per step of bench --config 5; 16: 0.713, and
                                                            //  half the slab bytes for the SGD kernel)
    while (s > 1 && (K % (s * kBgBK)) != 0) --s;           // whole k-tiles per slab
    return s;
}

// dst[i] = the ordered sum of `nslabs` contiguous slabs of `len` floats, on d->cur
static int launch_reduce_slabs(xq_dqn* d, const float* slabs, int nslabs, long long len, float* dst) {
    ProfScope ps(d, "reduce_slabs", (double)nslabs * len, 4.0 * (nslabs + 1) * len);
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)std::min<long long>((len + 255) / 256, 2048)), dim3(256), 0, d->cur, slabs, nslabs,
                       len, len, dst);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// dst[M][N] = sum over the batch: A(m,k) B(k,n), split-K slabs + ordered reduction.  a_bf / b_bf: the bf16 copies of the operands
// ([batch][M] / [batch][N]) for the bf16 loop.
template <int AL>
static int grad_gemm(xq_dqn* d, GemmArgs g, float* dst, const char* name, float* slab_base = nullptr,
                     xq_dqn::PendingSlab* defer = nullptr, const uint16_t* a_bf = nullptr, const uint16_t* b_bf = nullptr) {
    const bool use_bf = AL == L_MCONTIG && a_bf && b_bf && grad_bf16_ok(d, g.M, g.N, g.K);
    const int splits = use_bf ? grad_splits(d, g.M, g.N, g.K) : pick_splits(g.M, g.N, g.K);
    const long long len = (long long)g.M * g.N;
    float* slabs = slab_base;
    if (splits > 1 && !slabs) { XQ_TRY(d->slabs.reserve((size_t)splits * (size_t)len)); slabs = d->slabs; }
    float* C = splits > 1 ? slabs : dst;
    const long long slab_stride = splits > 1 ? len : 0;
    int used = splits;
    if (use_bf) {
        Bf16GemmArgs b; memset(&b, 0, sizeof b);
        b.M = g.M; b.N = g.N; b.K = g.K; b.A = a_bf; b.lda = g.lda; b.B = b_bf; b.ldb = g.ldb; b.k_chunk = g.K / splits;
        b.C = C; b.ldc = g.N; b.slab_stride = slab_stride;
        XQ_TRY((launch_bf16_gemm<L_MCONTIG, L_MCONTIG, BG_STORE>(d, b, splits, name)));
    } else {                               // 64-tiles: more tiles, fewer k-splits, cheaper ordered reduction
        g.C = C; g.ldc = g.N; g.slab_stride = slab_stride;
        XQ_TRY((launch_gemm<AL, L_MCONTIG, EPI_STORE>(d, g, splits, name, &used, true)));
    }
    if (splits <= 1) return XQ_OK;
    if (defer) { defer->src = slabs; defer->nslabs = used; defer->stride = len; return XQ_OK; }      // summed by the apply kernel
    return launch_reduce_slabs(d, slabs, used, len, dst);
}

struct BiasJobs {
    ColsumJobs J;
    BiasJobs() { memset(&J, 0, sizeof J); }
    void add(const float* X, long long ld, int C, float* dst) {
        const int k = J.njobs++;
        J.X[k] = X; J.ld[k] = ld; J.C[k] = C; J.dst[k] = dst;
    }
};
// defer != nullptr (fused_apply, TD step: the jobs are the hidden layers in ascending order, their destinations contiguous): the rows
// of partial sums are left to the SGD kernel as slabs — no final reduction launch
static int bias_grads(xq_dqn* d, BiasJobs& bj, int n, xq_dqn::PendingSlab* defer = nullptr) {
    ColsumJobs& J = bj.J;
    if (J.njobs == 0) return XQ_OK;
    J.n = n;
    J.R = std::max(1, std::min(64, n / 64));
    J.rows_per = (n + J.R - 1) / J.R;
    long long off = 0;
    int maxc = 0;
    for (int k = 0; k < J.njobs; ++k) { J.poff[k] = off; off += J.C[k]; maxc = std::max(maxc, J.C[k]); }
    J.wld = off;
    off *= J.R;
    XQ_TRY(d->bias_work.reserve((size_t)off));
    J.work = d->bias_work;
    if (defer) { defer->src = J.work; defer->nslabs = J.R; defer->stride = J.wld; }
    double tot = 0;
    for (int k = 0; k < J.njobs; ++k) tot += (double)n * J.C[k];
    if (d->tail_open) {                  // fused tail launch: the partial sums join the open grid (always deferred to the SGD kernel there)
        TailArgs& T = *d->tail;
        T.cj = J; T.cj_gx = (maxc + 63) / 64; T.cj_gy = J.R; T.n_colsum = T.cj_gx * T.cj_gy * J.njobs;
        d->tail_flops += tot; d->tail_bytes += 4.0 * tot;
        return XQ_OK;
    }
    ProfScope ps(d, "bias_grad_colsum", tot, 4.0 * tot);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((maxc + 63) / 64, J.R, J.njobs), dim3(256), 0, d->cur, J);
    XQ_HIP(hipGetLastError());
    if (defer) return XQ_OK;
    hipLaunchKernelGGL(colsum_final_kernel, dim3((maxc + 63) / 64, J.njobs), dim3(256), 0, d->cur, J);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// Launch shape of the segmented layer-0 sums (l0_grad_block): the column slab per block (grid z; wide layers keep the H = 256 shape), one
// accumulator set per wave while they fit in 60 KB of LDS, and the dynamic LDS of a block.  Widest H with lds <= 64 KB: 1132 at chunk 1024.
struct L0SegShape { int HS, nsets; size_t lds; };
static L0SegShape l0_seg_shape(int H, int chunk) {
    L0SegShape s;
    s.HS = (H > 256 && H % 256 == 0) ? 256 : H;
    s.nsets = 4;
    while (s.nsets > 1 && (size_t)s.nsets * 14 * s.HS * sizeof(float) > 60 * 1024) s.nsets >>= 1;
    s.lds = (size_t)s.nsets * 14 * s.HS * sizeof(float) + (size_t)chunk * sizeof(uint16_t);
    return s;
}

// layer 0: per-(square, piece) segmented sums of delta_0 rows (no dense one-hot product); launches on d->cur or joins the open fused
// grid.  defer != nullptr: the chunks' partial sums are left to the apply kernel as slabs — one kernel fewer on the critical chain
static int l0_gradient(xq_dqn* d, int n, float* dst, xq_dqn::PendingSlab* defer) {
    const int H = d->L[1];
    // samples per block (list entries hold 11 bits of sample index).  8192 samples: 1024 (2048 measured 56 against 52 us, round 2);
    // 16384 samples: 2048 — half the partial slabs for the SGD kernel to sum (41 -> 20 MB), bench --config 5 0.717 -> 0.704 ms
    const int chunk = l0_chunk_of(n);
    const int nchunks = (n + chunk - 1) / chunk;
    const long long len = (long long)kStateSize * H;
    float* out = dst;
    if (nchunks > 1) {
        XQ_TRY(d->slabs_l0.reserve((size_t)nchunks * (size_t)len));
        out = d->slabs_l0;
    }
    if (l0_mfma_shape(d, n)) {
        // the matrix-pipe form (xq_l0grad.hip.h): boards -> selector half-words, delta_0 -> three transposed bf16 planes, then
        // one-hot^T x planes on v_mfma_f32_16x16x32_bf16 — exact products, fp32 accumulation
        const int kpad = nchunks * chunk;
        XQ_TRY(ensure_l0_mfma(d, n));
        const size_t need_sel = l0sel_elems(kpad);
        const long long plane_stride = (long long)H * kpad;
        {
            LaunchNow now(d);                        // launches of their own, in front of the fused launch that is being assembled
            if (!d->l0_sel_done) {                   // (fused TD step of a net with >= 2 hidden layers: rode in the launch before this one)
                ProfScope ps(d, "l0_sel_words", 0.0, (double)n * 48 + 2.0 * need_sel);
                hipLaunchKernelGGL(l0_sel_kernel, dim3(kpad / 64), dim3(256), 0, d->cur, d->gboards, n, kpad, d->l0_sel, d->hot(), d->l0_cold_list.p,
                                   d->l0_cold_cnt.p);
            }
            if (!d->l0_split_done) {                 // (whole tiles: the delta product's epilogue wrote the planes)
                ProfScope ps(d, "l0_delta_split", 8.0 * n * H, (double)n * H * 4 + 6.0 * H * kpad);
                hipLaunchKernelGGL(delta_split_kernel, dim3(kpad / 64, H / 64), dim3(256), 0, d->cur, d->deltas[0], n, H, d->l0_planes, plane_stride, kpad);
            }
            d->l0_sel_done = d->l0_split_done = false;
        }
        XQ_HIP(hipGetLastError());
        // fused launch: the packed hot rows on the matrix pipe (48 tiles of 16 rows), the cold rows from their lists; alone: all 80 tiles
        const bool hot = d->tail_open;
        const size_t shmem = hot ? l0m_lds_bytes<true>() : l0m_lds_bytes<false>();
        const double fl = 2.0 * (hot ? kL0HotGroups * kL0HotGroupRows : 80 * 16) * (double)H * kpad * 3,
                     by = 6.0 * H * kpad + 2.0 * need_sel + 4.0 * nchunks * len;
        if (d->tail_open) {
            TailArgs& T = *d->tail;
            T.l0_n = n; T.l0_H = H; T.l0_chunk = chunk; T.l0_nch = nchunks; T.l0_partial = out;
            T.l0_sel = d->l0_sel; T.l0_planes = d->l0_planes; T.l0_plane_stride = plane_stride; T.l0_kpad = kpad; T.l0_ncb = H / kL0mCols;
            T.n_l0 = kL0HotGroups * (H / kL0mCols) * nchunks;
            T.l0_hot = d->hot(); T.l0_cold_list = d->l0_cold_list; T.l0_cold_cnt = d->l0_cold_cnt; T.l0_delta = d->deltas[0];
            T.n_l0cold = kL0ColdParts * nchunks;
            d->tail_flops += fl; d->tail_bytes += by;
            d->tail_lds = std::max(d->tail_lds, shmem);
        } else {
            ProfScope ps(d, "l0_grad_segsum", fl, by);
            XQ_TRY(ensure_max_dynamic_lds(l0_grad_mfma_kernel<0>, 64 * 1024));
            hipLaunchKernelGGL(l0_grad_mfma_kernel<0>, dim3(H / kL0mCols, 4, nchunks), dim3(256), shmem, d->cur, d->l0_sel, d->l0_planes, plane_stride,
                               kpad, H, chunk, out);
            XQ_HIP(hipGetLastError());
        }
    } else {
        ProfScope ps(d, "l0_grad_segsum", 2.0 * n * 32 * H, (double)n * (32.0 * H * 4 + 48) + 4.0 * nchunks * len);
        const L0SegShape shape = l0_seg_shape(H, chunk);
        const int HS = shape.HS, nsets = shape.nsets;
        const size_t shmem = shape.lds;              // (<= 64 KB: plan_gradients refused the step otherwise, before its first gradient launch)
        if (d->tail_open) {              // fused tail launch
            TailArgs& T = *d->tail;
            T.l0_boards = d->gboards; T.l0_delta = d->deltas[0]; T.l0_n = n; T.l0_H = H; T.l0_HS = HS; T.l0_chunk = chunk; T.l0_nsets = nsets;
            T.l0_nch = nchunks; T.l0_partial = out; T.n_l0 = kSquares * nchunks * (H / HS);
            d->tail_flops += 2.0 * n * 32 * H; d->tail_bytes += (double)n * (32.0 * H * 4 + 48) + 4.0 * nchunks * len;
            d->tail_lds = std::max(d->tail_lds, shmem);
        } else {
        if (shmem > 48 * 1024) XQ_TRY(ensure_max_dynamic_lds(l0_grad_kernel, 64 * 1024));
        hipLaunchKernelGGL(l0_grad_kernel, dim3(kSquares, nchunks, H / HS), dim3(256), shmem, d->cur, d->gboards, d->deltas[0], n, H, HS,
                           chunk, nsets, out);
        XQ_HIP(hipGetLastError());
        }
    }
    if (nchunks <= 1) return XQ_OK;
    if (defer) { defer->src = d->slabs_l0; defer->nslabs = nchunks; defer->stride = len; return XQ_OK; }
    return launch_reduce_slabs(d, d->slabs_l0, nchunks, len, dst);
}

// Which segments go four elements to a thread (t.vec4: every pointer 16-byte aligned — the bf16 shadow, where there is one, is stored in
// 8-byte pieces — len and slab stride multiples of 4; `state`: so is the offset into Adam's m and v), and the x size of a grid
// (blocks, segments) of 256 threads that covers the longest segment, capped at 1024.
// soft: the target net's pointers of a SOFT kernel and their shadows count like dst and dst_bf.
static unsigned seg_grid(SegTable& t, bool state, const SoftArgs* soft = nullptr) {
    long long mx = 0;
    for (int i = 0; i < t.nseg; ++i) {
        uintptr_t bits = (uintptr_t)t.dst[i] | (uintptr_t)t.src[i] | ((uintptr_t)t.dst_bf[i] << 1);
        if (soft) bits |= (uintptr_t)soft->tgt[i] | ((uintptr_t)soft->tgt_bf[i] << 1);
        t.vec4[i] = (bits & 15) == 0 && (t.len[i] & 3) == 0 && (t.nslabs[i] <= 0 || (t.stride[i] & 3) == 0) &&
                    (!state || (t.state_off[i] & 3) == 0);
        mx = std::max(mx, t.vec4[i] ? t.len[i] / 4 : t.len[i]);
    }
    return (unsigned)std::max<long long>(1, std::min<long long>((mx + 255) / 256, 1024));
}

// soft (never with reduce_only): the SOFT form of the same kernel, which moves the target net's segments in the same walk.
static int sgd_apply(xq_dqn* d, SegTable t, double alpha, const ClipArgs* clip = nullptr, const SoftArgs* soft = nullptr) {
    const unsigned bx = seg_grid(t, false, soft);
    ProfScope ps(d, t.reduce_only ? "reduce_slabs" : "sgd_apply", 0, 0, true);
    if (soft && clip) hipExtLaunchKernelGGL(sgd_segments_clip_soft_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, (float)alpha, *clip, *soft);
    else if (soft) hipExtLaunchKernelGGL(sgd_segments_soft_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, (float)alpha, *soft);
    else if (clip) hipExtLaunchKernelGGL(sgd_segments_clip_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, (float)alpha, *clip);
    else
    hipExtLaunchKernelGGL(sgd_segments_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, (float)alpha);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// The same table through adam_segments_kernel: step t of Adam with the handle's betas and eps.  The bias corrections are taken on the
// host in double and handed over as floats.
static int adam_apply(xq_dqn* d, SegTable t, double lr, double grad_scale, const ClipArgs* clip = nullptr, const SoftArgs* soft = nullptr) {
    const unsigned bx = seg_grid(t, true, soft);
    d->opt_t += 1;
    const double tt = (double)d->opt_t;
    AdamArgs A;
    A.m = d->adam_m; A.v = d->adam_v;
    A.b1 = (float)d->opt_b1; A.omb1 = (float)(1.0 - d->opt_b1);
    A.b2 = (float)d->opt_b2; A.omb2 = (float)(1.0 - d->opt_b2);
    A.eps = (float)d->opt_eps;
    A.a = (float)(lr / (1.0 - std::pow(d->opt_b1, tt)));
    A.rbc2 = (float)(1.0 / std::sqrt(1.0 - std::pow(d->opt_b2, tt)));
    A.gs = (float)grad_scale;
    ProfScope ps(d, "adam_apply", 0, 0, true);
    if (soft && clip) hipExtLaunchKernelGGL(adam_segments_clip_soft_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, A, *clip, *soft);
    else if (soft) hipExtLaunchKernelGGL(adam_segments_soft_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, A, *soft);
    else if (clip) hipExtLaunchKernelGGL(adam_segments_clip_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, A, *clip);
    else
    hipExtLaunchKernelGGL(adam_segments_kernel, dim3(bx, t.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, t, A);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// Gradient clipping, in front of the apply: the squares of the whole gradient summed in fp64 into one partial per block (grad_norm_kernel,
// fixed grid), pending slabs summed into the gradient buffer on the way.  On return the table reads the buffer and nothing is pending;
// the coefficient is formed inside the apply kernel from the partials, so nothing comes back to the host.
static int grad_norm(xq_dqn* d, SegTable& t, double grad_scale, ClipArgs* C) {
    if (t.nseg * kNormBlocks > kNormMaxPartials) return fail(XQ_ERR_RUNTIME, "grad_norm: %d segments", t.nseg);
    float* G = d->grads_td;
    SegTable n = t;
    double bytes = 0;
    for (int i = 0; i < n.nseg; ++i) {
        n.dst[i] = G + n.state_off[i];
        n.dst_bf[i] = nullptr;                       // the norm reads and writes gradients only: no shadow in its alignment rule
        bytes += 4.0 * n.len[i] * (n.nslabs[i] > 0 ? n.nslabs[i] + 1 : 1);
    }
    seg_grid(n, false);                              // its vec4[]; the grid is fixed (kNormBlocks)
    {
        ProfScope ps(d, "grad_norm", 0, bytes, true);
        hipExtLaunchKernelGGL(grad_norm_kernel, dim3(kNormBlocks, n.nseg), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, n, d->clip_partials.p);
        XQ_HIP(hipGetLastError());
    }
    for (int i = 0; i < t.nseg; ++i) { t.src[i] = G + t.state_off[i]; t.nslabs[i] = 0; t.stride[i] = 0; }
    C->partials = d->clip_partials; C->npart = t.nseg * kNormBlocks;
    C->max_norm = d->clip_max_norm; C->abs_scale = std::fabs(grad_scale);
    C->rec = d->clip_rec;
    return XQ_OK;
}

static void layout_td_grads(xq_dqn* d) {
    size_t off = 0;
    d->g_w0 = off; off += (size_t)d->L[0] * d->L[1];
    for (int l = 1; l + 1 < d->nl; ++l) { d->g_wh[l] = off; off += (size_t)d->L[l] * d->L[l + 1]; }
    d->g_wout = off; off += (size_t)96 * d->hlast();
    d->g_bout = off; off += 96;                      // directly behind the output rows: one ordered reduction fills both
    for (int l = 0; l + 1 < d->nl; ++l) { d->g_bh[l] = off; off += (size_t)d->L[l + 1]; }
    d->n_grads_td = off;
}
// a TD step left partial-sum slabs for its apply_grads to add (fused_apply)
static bool td_step_pending(const xq_dqn* d) { return d->pend_w0.nslabs > 0 || d->pend_wout.nslabs > 0 || d->pend_bh.nslabs > 0; }
// The segments a TD step touches, in THE order of every table built from them (the order is part of the clip norm's association):
// W0^T, the hidden weights, output rows 0..95, the hidden biases (contiguous in both layouts), the output biases.  f(parameters, their
// bf16 shadow or nullptr, offset in the gradient buffer, length, the segment's pending-slab slot) — f empties the slot it takes.
template <class F>
static void for_td_segments(xq_dqn* d, F f) {
    const bool bf = d->bf16();
    const int top = d->nl - 1;
    f(d->w0t(0), bf ? d->wl_bf(0, 0) : nullptr, d->g_w0, (long long)d->L[0] * d->L[1], d->pend_w0);
    for (int l = 1; l < top; ++l) f(d->wl(0, l), bf ? d->wl_bf(0, l) : nullptr, d->g_wh[l], (long long)d->L[l] * d->L[l + 1], d->pend_hidden[l]);
    f(d->wl(0, top), bf ? d->wl_bf(0, top) : nullptr, d->g_wout, 96LL * d->hlast(), d->pend_wout);
    f(d->bl(0, 0), (uint16_t*)nullptr, d->g_bh[0], (long long)d->bo[top], d->pend_bh);
    f(d->bl(0, top), (uint16_t*)nullptr, d->g_bout, 96LL, d->pend_bout);
}
// The same segments of the target net, in the same order: what a SOFT apply kernel walks beside the table built from for_td_segments.
static void soft_td_segments(const xq_dqn* d, SoftArgs* Z) {
    const bool bf = d->bf16();
    const int top = d->nl - 1;
    int k = 0;
    auto add = [&](float* t, uint16_t* tb) { Z->tgt[k] = t; Z->tgt_bf[k] = tb; ++k; };
    add(d->w0t(1), bf ? d->wl_bf(1, 0) : nullptr);
    for (int l = 1; l < top; ++l) add(d->wl(1, l), bf ? d->wl_bf(1, l) : nullptr);
    add(d->wl(1, top), bf ? d->wl_bf(1, top) : nullptr);
    add(d->bl(1, 0), nullptr);
    add(d->bl(1, top), nullptr);
}
// What a write of params[] or params_bf[] makes stale.  Every site that queues one calls this exactly once and touches none of the derived
// state itself; how the bf16 shadow is brought up to date stays at the site (the mechanisms differ).
//   write                                                        params_version  screen rows >= 96         kept sums of select  tgt_rest_synced
//   ONLINE_WHOLE  set_params(0), so load_model; backpropagate    +1              invalid if the online's   dropped              false
//   TARGET_HOST   set_params(1)                                  +1              invalid if the target's   kept                 false
//   TARGET_COPY   target := online (update_target)               +1              invalid if the target's   kept                 true
//   TARGET_BLEND  whole-buffer soft update (soft_target_whole)   +1              invalid if the target's   kept                 unchanged
//   TD_SEGMENTS   apply_grads (fused soft form: the target's     +1              kept (only rows 0..95     dropped, pays/calls  unchanged
//                 TD segments too)                                               move)                     rolled over
//   BF16_SHADOW   set_precision rebuilds the shadow              +1              kept                      kept                 unchanged
// (params_version: is the trainer's `params` mark still current?  The kept layer-0 sums are the online net's alone.)
// Order: what invalidates comes before the write is queued, so a launch that fails leaves the derived state on the conservative side.
// TARGET_COPY is the one row that asserts something: its site calls behind the copy, once that was queued successfully.
enum class ParamWrite { ONLINE_WHOLE, TARGET_HOST, TARGET_COPY, TARGET_BLEND, TD_SEGMENTS, BF16_SHADOW };
static void params_written(xq_dqn* d, ParamWrite what) {
    d->params_version += 1;
    switch (what) {
    case ParamWrite::ONLINE_WHOLE:  d->scr.rows_rewritten(XQ_NET_ONLINE); d->sel_invalidate(); d->tgt_rest_synced = false; break;
    case ParamWrite::TARGET_HOST:   d->scr.rows_rewritten(XQ_NET_TARGET); d->tgt_rest_synced = false; break;
    case ParamWrite::TARGET_COPY:   d->scr.rows_rewritten(XQ_NET_TARGET); d->tgt_rest_synced = true; break;
    case ParamWrite::TARGET_BLEND:  d->scr.rows_rewritten(XQ_NET_TARGET); break;
    case ParamWrite::TD_SEGMENTS:   d->sel_invalidate(); for (auto& K : d->sel_keep) { K.pays = K.calls >= 2; K.calls = 0; } break;
    case ParamWrite::BF16_SHADOW:   break;
    }
}

// One soft update of the whole target net from the online buffer (soft_target_kernel), on the handle's stream: every parameter and the
// shadow of every weight.
static int soft_target_whole(xq_dqn* d, double tau) {
    const long long n = (long long)(d->nw + d->nb);
    const float* p = d->params[0];
    float* t = d->params[1];
    uint16_t* tb = d->bf16() ? d->params_bf[1].p : nullptr;
    const int vec = ((((uintptr_t)p | (uintptr_t)t) & 15) == 0 && ((uintptr_t)tb & 7) == 0) ? 1 : 0;
    const long long items = vec ? (n >> 2) + 3 : n;
    const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((items + 255) / 256, 2048));
    params_written(d, ParamWrite::TARGET_BLEND);
    ProfScope ps(d, "soft_target", 2.0 * n, 12.0 * n + (tb ? 2.0 * d->nw : 0.0), true);
    hipExtLaunchKernelGGL(soft_target_kernel, dim3(blocks), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, p, t, tb, n, (long long)d->nw,
                          (float)tau, vec);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// view_boards_kernel on `stream` (xq_internal.h): the sides from side_dev or, with meta_dev, from bit 16 of meta[b].x
int view_boards_launch(const uint32_t* boards_dev, const uint8_t* side_dev, const uint4* meta_dev, int n, uint32_t* out_dev,
                       hipStream_t stream) {
    if (!boards_dev || !out_dev || (!side_dev && !meta_dev) || n < 0) return fail(XQ_ERR_INVALID_ARGUMENT, "view_boards: bad argument");
    if (!n) return XQ_OK;
    hipLaunchKernelGGL(view_boards_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, boards_dev, side_dev, meta_dev, n, out_dev);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

}  // namespace xq

using namespace xq;

// =================================================================================================================
// C ABI — dqn
// =================================================================================================================
extern "C" {

static int dqn_init(xq_dqn* d, const int* layer_sizes, int n_sizes, double learning_rate, double gamma, uint64_t seed,
                    void* hip_stream);
static int refresh_shadow(xq_dqn* d, int net);

int xq_dqn_create(const int* layer_sizes, int n_sizes, double learning_rate, double gamma, uint64_t seed, void* hip_stream,
                  xq_dqn** out) {
    if (!out || !layer_sizes) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_create: null pointer");
    if (n_sizes < 2) return fail(XQ_ERR_INVALID_ARGUMENT, "NeuralNetwork must have at least two layers (input and output).");
    if (n_sizes < 3 || n_sizes > XQ_MAX_LAYERS + 1)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn supports 1..%d hidden layers (got %d sizes)", XQ_MAX_LAYERS - 1, n_sizes);
    for (int i = 0; i < n_sizes; ++i)
        if (layer_sizes[i] <= 0) return fail(XQ_ERR_INVALID_ARGUMENT, "layer size must be positive");
    int c = 0;
    XQ_TRY(xq_device_count(&c));
    if (c == 0) return fail(XQ_ERR_NO_DEVICE, "no HIP device: libxqhip has no CPU fallback");
    xq_dqn* d = new xq_dqn();
    const int rc = dqn_init(d, layer_sizes, n_sizes, learning_rate, gamma, seed, hip_stream);
    if (rc != XQ_OK) { xq_dqn_destroy(d); return rc; }      // whatever it had allocated, created or recorded goes with the handle
    *out = d;
    return XQ_OK;
}

static int dqn_init(xq_dqn* d, const int* layer_sizes, int n_sizes, double learning_rate, double gamma, uint64_t seed,
                    void* hip_stream) {
    d->ns = n_sizes; d->nl = n_sizes - 1;
    for (int i = 0; i < n_sizes; ++i) d->L[i] = layer_sizes[i];
    for (int l = 0; l < d->nl; ++l) {                       // offsets, dqn.cu:125-140
        d->wo[l] = d->nw; d->bo[l] = d->nb;
        d->nw += (size_t)d->L[l] * d->L[l + 1];
        d->nb += (size_t)d->L[l + 1];
    }
    d->lr = learning_rate; d->gamma = gamma; d->seed = seed;
    XQ_TRY(d->stream.open(hip_stream));
    d->cur = d->stream;
    {
        hipDeviceProp_t prop; int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            d->ncu = prop.multiProcessorCount;
    }
    XQ_TRY(d->side.open_owned(hipStreamNonBlocking));
    for (Event* ev : {&d->ev_fork, &d->ev_join, &d->ev_delta, &d->ev_qmax}) XQ_TRY(ev->create(stream_event_flags()));
    // + 128 rows of the widest layer: the persistent column-max GEMM reads whole 128-row tiles of W_out (rows beyond the
    // last output are masked in its epilogue, but must be readable)
    int widest = 0;
    for (int i = 0; i < n_sizes; ++i) widest = std::max(widest, layer_sizes[i]);
    const size_t pad = (size_t)128 * widest;
    for (auto& p : d->params) {
        XQ_TRY(p.alloc(d->nw + d->nb + pad));
        XQ_HIP(hipMemsetAsync(p, 0, p.n * sizeof(float), d->stream));
    }
    layout_td_grads(d);
    XQ_TRY(d->grads_td.alloc(d->n_grads_td));
    XQ_HIP(hipMemsetAsync(d->grads_td, 0, d->n_grads_td * sizeof(float), d->stream));
    // initializeHostWeightsAndBiases (dqn.cu:96-123): U(-0.05, 0.05) in [layer][out][in] order, biases 0
    std::vector<double> w(d->nw), b(d->nb, 0.0);
    std::mt19937_64 gen(seed);
    std::uniform_real_distribution<double> dis(-0.05, 0.05);
    for (size_t i = 0; i < d->nw; ++i) w[i] = dis(gen);
    XQ_TRY(xq_dqn_set_params(d, XQ_NET_ONLINE, w.data(), b.data()));
    return xq_dqn_update_target(d);                          // DQN ctor, dqn.cpp:18
}

int xq_dqn_destroy(xq_dqn* d) {
    if (!d) return XQ_OK;
    d->prof.collect();                                       // (waits for its brackets' events: both streams still exist)
    d->side.close();
    d->stream.close();
    delete d->tail;
    delete d;                                                // the buffers and events go here: behind the synchronises above
    return XQ_OK;
}

int xq_dqn_stream(const xq_dqn* d, void** s) {
    if (!d || !s) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    *s = (void*)(hipStream_t)d->stream;
    return XQ_OK;
}

int xq_dqn_num_params(const xq_dqn* d, size_t* nw, size_t* nb) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (nw) *nw = d->nw;
    if (nb) *nb = d->nb;
    return XQ_OK;
}

int xq_dqn_set_params(xq_dqn* d, int net, const double* w, const double* b) {
    if (!d || !w || !b || net < 0 || net > 1) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_params: bad argument");
    std::vector<float> p(d->nw + d->nb);
    const int L0 = d->L[0], L1 = d->L[1];
    for (int j = 0; j < L1; ++j)
        for (int i = 0; i < L0; ++i) p[(size_t)i * L1 + j] = (float)w[(size_t)j * L0 + i];     // W0 [out][in] -> W0^T
    for (size_t i = d->wo[1]; i < d->nw; ++i) p[i] = (float)w[i];
    for (size_t i = 0; i < d->nb; ++i) p[d->nw + i] = (float)b[i];
    XQ_HIP(hipStreamSynchronize(d->stream));
    params_written(d, net == XQ_NET_ONLINE ? ParamWrite::ONLINE_WHOLE : ParamWrite::TARGET_HOST);
    XQ_HIP(hipMemcpy(d->params[net], p.data(), p.size() * sizeof(float), hipMemcpyHostToDevice));
    XQ_TRY(refresh_shadow(d, net));
    XQ_HIP(hipStreamSynchronize(d->stream));                    // a host-buffer entry point returns with the parameters in place
    return XQ_OK;
}

int xq_dqn_get_params(xq_dqn* d, int net, double* w, double* b) {
    if (!d || net < 0 || net > 1) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_get_params: bad argument");
    std::vector<float> p(d->nw + d->nb);
    XQ_HIP(hipStreamSynchronize(d->stream));
    XQ_HIP(hipMemcpy(p.data(), d->params[net], p.size() * sizeof(float), hipMemcpyDeviceToHost));
    const int L0 = d->L[0], L1 = d->L[1];
    if (w) {
        for (int j = 0; j < L1; ++j)
            for (int i = 0; i < L0; ++i) w[(size_t)j * L0 + i] = (double)p[(size_t)i * L1 + j];
        for (size_t i = d->wo[1]; i < d->nw; ++i) w[i] = (double)p[i];
    }
    if (b) for (size_t i = 0; i < d->nb; ++i) b[i] = (double)p[d->nw + i];
    return XQ_OK;
}

int xq_dqn_update_target(xq_dqn* d) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    ProfScope ps(d, "target_sync_copy", 0, 8.0 * (d->nw + d->nb));
    XQ_HIP(hipMemcpyAsync(d->params[1], d->params[0], (d->nw + d->nb) * sizeof(float), hipMemcpyDeviceToDevice, d->stream));
    params_written(d, ParamWrite::TARGET_COPY);
    if (d->bf16())
        XQ_HIP(hipMemcpyAsync(d->params_bf[1], d->params_bf[0], d->nw * sizeof(uint16_t), hipMemcpyDeviceToDevice, d->stream));
    return XQ_OK;
}

static int refresh_shadow(xq_dqn* d, int net) {
    if (!d->bf16()) return XQ_OK;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(1024), dim3(256), 0, d->stream, d->params[net], d->params_bf[net], (long long)d->nw);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

int xq_dqn_set_l0_derive(xq_dqn* d, int on) {
    if (d) d->sel_invalidate();
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    d->l0_derive = on != 0;
    return XQ_OK;
}

int xq_dqn_set_l0_grad_mode(xq_dqn* d, int mode) {
    if (!d || (mode != 0 && mode != 1)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_l0_grad_mode: 0 (segmented sums) or 1 (matrix pipe)");
    d->l0_mfma = mode == 1;
    return XQ_OK;
}

int xq_dqn_set_refine_stage(xq_dqn* d, int mode) {
    if (!d || mode < -1 || mode > 1) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_refine_stage: -1 (by the screen's counters), 0 (never) or 1 (whenever the launch has room)");
    d->scr.refine_stage = mode;
    return XQ_OK;
}

int xq_dqn_set_td_tail(xq_dqn* d, int on) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    d->td_tail = on != 0;
    return XQ_OK;
}

int xq_dqn_set_exchange_overlap(xq_dqn* d, int mode) {
    if (!d || mode < -1 || mode > 1) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_exchange_overlap: mode -1, 0 or 1");
    d->exchange_overlap = mode;
    return XQ_OK;
}

int xq_dqn_set_qmax_mode(xq_dqn* d, int mode) {
    if (!d || (mode != XQ_QMAX_FULL && mode != XQ_QMAX_SCREENED)) return fail(XQ_ERR_INVALID_ARGUMENT, "bad qmax mode");
    d->scr.set_mode(mode);
    return XQ_OK;
}

int xq_dqn_qmax_stats(xq_dqn* d, uint64_t stats[4]) {
    if (!d || !stats) return fail(XQ_ERR_INVALID_ARGUMENT, "null");
    unsigned long long h[2] = {0, 0};
    XQ_TRY(d->scr.totals(h));
    stats[0] = d->scr.host_steps; stats[1] = d->scr.host_samples; stats[2] = h[0]; stats[3] = h[1];
    return XQ_OK;
}

int xq_dqn_qmax_guard(xq_dqn* d, uint64_t* fallbacks, int* hold_steps_left) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (fallbacks) *fallbacks = d->scr.fallbacks;
    if (hold_steps_left) *hold_steps_left = d->scr.hold;
    return XQ_OK;
}

int xq_dqn_set_precision(xq_dqn* d, int precision) {
    if (!d || (precision != XQ_PRECISION_F32 && precision != XQ_PRECISION_BF16 && precision != XQ_PRECISION_BF16_FULL))
        return fail(XQ_ERR_INVALID_ARGUMENT, "bad precision");
    if (td_step_pending(d))
        return fail(XQ_ERR_RUNTIME, "xq_dqn_set_precision: a TD step is waiting for its apply_grads");
    if (precision != XQ_PRECISION_F32) {
        for (int l = 1; l <= d->nl - 1; ++l)
            if (d->L[l] & 1) return fail(XQ_ERR_INVALID_ARGUMENT, "bf16 Q-net needs even hidden widths (layer %d has %d)", l, d->L[l]);
        int widest = 0;
        for (int i = 0; i < d->ns; ++i) widest = std::max(widest, d->L[i]);
        const size_t pad = (size_t)128 * widest;             // whole-tile reads of the persistent GEMM, like params[]
        for (auto& p : d->params_bf) XQ_TRY(reserve_zeroed(p, d->nw + pad, d->stream));      // (first call only)
    }
    d->precision = precision;
    params_written(d, ParamWrite::BF16_SHADOW);
    XQ_TRY(refresh_shadow(d, 0));
    return refresh_shadow(d, 1);
}

// dense-state chain: a_1 via GEMM against W0^T; outs as in chain_boards
static int chain_dense(xq_dqn* d, int net, const float* x, int n, float* const* outs) {
    GemmArgs g; memset(&g, 0, sizeof g);
    g.M = n; g.N = d->L[1]; g.K = d->L[0];
    g.A = x; g.lda = d->L[0];
    g.B = d->w0t(net); g.ldb = d->L[1];
    g.C = outs[0]; g.ldc = d->L[1];
    g.bias = d->bl(net, 0);
    g.libm_tanh = !XQ_L0_FAST_TANH;      // layer 0 takes the SAME tanh on both routes (tanh_l0 in the packed-board gather kernels): a dense
                                         // one-hot and the board it encodes then differ by summation order only
    XQ_TRY((launch_gemm<L_KCONTIG, L_MCONTIG, EPI_BIAS_TANH>(d, g, 1, "gemm_l0_dense_fwd")));
    const ChainJob job{net, nullptr, outs};          // the hidden layers: the fp32 tile product of chain_boards with one chain
    bool aligned;
    for (int l = 1; l + 1 < d->nl; ++l)
        XQ_TRY((launch_gemm<L_KCONTIG, L_KCONTIG, EPI_BIAS_TANH>(d, hidden_f32_args(d, &job, 1, l, n, &aligned), 1, "gemm_hidden_fwd")));
    return XQ_OK;
}

static int upload_dense(xq_dqn* d, const double* src, size_t count, DevBuf<float>& dev) {
    XQ_TRY(dev.reserve(count));
    std::vector<float> tmp(count);
    for (size_t i = 0; i < count; ++i) tmp[i] = (float)src[i];
    XQ_HIP(hipStreamSynchronize(d->stream));
    XQ_HIP(hipMemcpy(dev, tmp.data(), count * sizeof(float), hipMemcpyHostToDevice));
    return XQ_OK;
}

int xq_dqn_forward(xq_dqn* d, int net, const double* states, int n, double* q_host) {
    if (!d || !states || !q_host || n <= 0 || net < 0 || net > 1)
        return fail(XQ_ERR_INVALID_ARGUMENT, "Input size does not match network input layer size.");
    XQ_TRY(ensure_capacity(d, n));
    XQ_TRY(upload_dense(d, states, (size_t)n * d->L[0], d->xdense));
    XQ_TRY(d->qfull.reserve((size_t)n * d->nout()));
    float* outs[XQ_MAX_LAYERS];
    for (int l = 0; l + 1 < d->nl; ++l) outs[l] = d->acts[l];
    XQ_TRY(chain_dense(d, net, d->xdense, n, outs));
    XQ_TRY(q_head(d, net, outs[d->nl - 2], n, d->nout(), d->qfull, d->nout(), "gemm_q_full"));
    std::vector<float> q((size_t)n * d->nout());
    XQ_HIP(hipMemcpyAsync(q.data(), d->qfull, q.size() * sizeof(float), hipMemcpyDeviceToHost, d->stream));
    XQ_HIP(hipStreamSynchronize(d->stream));
    for (size_t i = 0; i < q.size(); ++i) q_host[i] = (double)q[i];
    return XQ_OK;
}

int xq_dqn_forward_boards_dev(xq_dqn* d, int net, const uint32_t* boards_dev, int n, int n_out, float* q_dev, int ldq) {
    if (!d || !boards_dev || !q_dev || n <= 0 || net < 0 || net > 1 || n_out <= 0 || n_out > d->nout() || ldq < n_out)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_forward_boards_dev: bad argument");
    XQ_TRY(ensure_capacity(d, n));
    XQ_TRY(ensure_ext_capacity(d, n, false));
    float* outs[XQ_MAX_LAYERS];
    uint16_t* outs_bf[XQ_MAX_LAYERS] = {nullptr};
    chain_views(d, d->acts, d->acts_bf, XQ_MAX_LAYERS, true, outs, outs_bf);
    ChainJob job{net, boards_dev, outs, outs_bf, nullptr};
    XQ_TRY(chain_boards(d, &job, 1, explicit_slots(nullptr), n));
    return q_head(d, net, outs[d->nl - 2], n, n_out, q_dev, ldq, n_out <= 96 ? "gemm_q90_select" : "gemm_q_full",
                  d->bf16() ? outs_bf[d->nl - 2] : nullptr);
}

int xq_dqn_select_q_dev(xq_dqn* d, const uint32_t* boards_dev, int n, float* q_dev) {
    if (!d || !boards_dev || !q_dev || n <= 0) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_select_q_dev: bad argument");
    float* q = nullptr;
    int stride = 0;
    XQ_TRY(dqn_q90_boards(d, boards_dev, n, &q, &stride, nullptr, nullptr));
    XQ_HIP(hipMemcpyAsync(q_dev, q, (size_t)n * 96 * sizeof(float), hipMemcpyDeviceToDevice, d->stream));
    return XQ_OK;
}

int xq_dqn_backpropagate(xq_dqn* d, const double* states, const double* targets, int n, double lr, double grad_scale, int mode) {
    if (!d || !states || !targets || n <= 0) return fail(XQ_ERR_INVALID_ARGUMENT, "Input size does not match network input layer size.");
    if (mode != XQ_BACKPROP_REFERENCE && mode != XQ_BACKPROP_TEXTBOOK) return fail(XQ_ERR_INVALID_ARGUMENT, "bad backprop mode");
    // the pending step's partial sums live in bias_work and slabs, which bias_grads and grad_gemm below write (and reserve() may move)
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_backpropagate: a TD step is waiting for its apply_grads");
    if (mode == XQ_BACKPROP_REFERENCE) XQ_TRY(check_reference_topology(d));
    XQ_TRY(ensure_capacity(d, n));
    const int NO = d->nout();
    XQ_TRY(upload_dense(d, states, (size_t)n * d->L[0], d->xdense));
    XQ_TRY(upload_dense(d, targets, (size_t)n * NO, d->tfull));
    XQ_TRY(d->qfull.reserve((size_t)n * NO));
    XQ_TRY(d->grads_full.reserve(d->nw + d->nb));
    float* outs[XQ_MAX_LAYERS];
    for (int l = 0; l + 1 < d->nl; ++l) outs[l] = d->acts[l];
    XQ_TRY(chain_dense(d, XQ_NET_ONLINE, d->xdense, n, outs));
    XQ_TRY(q_head(d, XQ_NET_ONLINE, outs[d->nl - 2], n, NO, d->qfull, NO, "gemm_q_full"));
    const long long total = (long long)n * NO;
    hipLaunchKernelGGL(out_delta_dense_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0,
                       d->cur, d->qfull, d->tfull, total, d->tfull);      // delta overwrites the target buffer
    XQ_HIP(hipGetLastError());
    const float* dout = d->tfull;
    XQ_TRY(hidden_deltas(d, n, dout, NO, NO, mode));
    // gradients, full layout = parameter layout
    float* gw = d->grads_full;
    float* gb = d->grads_full + d->nw;
    BiasJobs bj;
    {   // layer 0: gW0^T[in][out] = X^T delta_0
        GemmArgs g; memset(&g, 0, sizeof g);
        g.M = d->L[0]; g.N = d->L[1]; g.K = n;
        g.A = d->xdense; g.lda = d->L[0];
        g.B = d->deltas[0]; g.ldb = d->L[1];
        XQ_TRY((grad_gemm<L_MCONTIG>(d, g, gw, "gemm_grad_l0_dense")));
        bj.add(d->deltas[0], d->L[1], d->L[1], gb + d->bo[0]);
    }
    for (int l = 1; l < d->nl; ++l) {   // gW_l[out][in] = delta_l^T a_l
        const float* dl = (l == d->nl - 1) ? dout : d->deltas[l];
        const int ldd = (l == d->nl - 1) ? NO : d->L[l + 1];
        GemmArgs g; memset(&g, 0, sizeof g);
        g.M = d->L[l + 1]; g.N = d->L[l]; g.K = n;
        g.A = dl; g.lda = ldd;
        g.B = d->acts[l - 1]; g.ldb = d->L[l];
        XQ_TRY((grad_gemm<L_MCONTIG>(d, g, gw + d->wo[l], "gemm_grad_dense")));
        bj.add(dl, ldd, d->L[l + 1], gb + d->bo[l]);
    }
    XQ_TRY(bias_grads(d, bj, n));
    SegTable t; memset(&t, 0, sizeof t);
    t.nseg = 1; t.dst[0] = d->params[0]; t.src[0] = d->grads_full; t.len[0] = (long long)(d->nw + d->nb);
    params_written(d, ParamWrite::ONLINE_WHOLE);       // dense update: every row changes, and the target net, which this never touches, no longer has them
    XQ_TRY(sgd_apply(d, t, lr * grad_scale));
    XQ_TRY(refresh_shadow(d, XQ_NET_ONLINE));          // bf16 Q-net: every later bf16 forward must see the updated weights
    XQ_HIP(hipStreamSynchronize(d->stream));
    return XQ_OK;
}

// prioritized replay hooks of one TD step (device pointers owned by the replay ring; nullptr = uniform replay)
struct PerOpts {
    const float* is_w; const float* is_wmax;
    float* prio; unsigned* pmax_live;
    float eps, alpha;
};
static int td_grads_impl(xq_dqn* d, const uint32_t* boards, const uint32_t* next_boards, const int32_t* action_to,
                         const float* reward, const uint8_t* done, SlotSrc slots, int n, int td_net, int mode, const PerOpts* per,
                         const float* discount = nullptr, const uint8_t* next_player = nullptr);

int xq_dqn_td_grads(xq_dqn* d, const uint32_t* boards, const uint32_t* next_boards, const int32_t* action_to,
                    const float* reward, const uint8_t* done, const int32_t* slots, int n, int td_net, int mode) {
    return td_grads_impl(d, boards, next_boards, action_to, reward, done, explicit_slots(slots), n, td_net, mode, nullptr);
}
int xq_dqn_td_grads_sided(xq_dqn* d, const uint32_t* boards, const uint32_t* next_boards, const int32_t* action_to,
                          const float* reward, const uint8_t* done, const uint8_t* next_player, const int32_t* slots, int n, int td_net, int mode) {
    if (!next_player) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_td_grads_sided: null next_player");
    return td_grads_impl(d, boards, next_boards, action_to, reward, done, explicit_slots(slots), n, td_net, mode, nullptr, nullptr, next_player);
}

// ---- the gradient half of a TD step: one description of each gradient, emitted in two orders -----------------------------------
// Each helper below is the one place that knows its gradient's shapes, operands, accounting and pending slot; like bias_grads and
// l0_gradient it appends to the open fused grid (TailGrid) or launches on d->cur.  side_gradients and tail_gradients are the two orders.

// Where the partial-sum slabs of a step's output-layer and hidden weight gradients go in d->slabs.  defer: they wait for the apply
// kernel (or reduce_pending), so every segment has a region of its own; otherwise each launch is followed by its ordered sum and they
// use one region in turn.  (Layer 0 and the hidden biases have buffers of their own: slabs_l0, bias_work.)
struct GradPlan {
    bool defer;
    int out_chunks;  long long len_out;  size_t out_lds;     // output-layer sums: blocks of kOutGradChunk samples, [96][Hl] + [96] per slab
    size_t off_out, off_h[XQ_MAX_LAYERS];
};
// samples per block of the output-layer sums: small chunks level the load between popular and rare destination squares
// (1024: 21.7 us and a side stream that ends with the critical one; 256: 16.4 us, step -10 us)
static const int kOutGradChunk = 256;
static int plan_gradients(xq_dqn* d, int n, bool defer, GradPlan* P) {
    const int Hl = d->hlast();
    memset(P, 0, sizeof *P);
    P->defer = defer;
    P->out_chunks = (n + kOutGradChunk - 1) / kOutGradChunk;
    P->len_out = 96LL * Hl + 96;
    P->out_lds = (size_t)16 * Hl * sizeof(float) + (size_t)kOutGradChunk * sizeof(uint16_t);
    if (P->out_lds > 64 * 1024 || (Hl & 3))
        return fail(XQ_ERR_INVALID_ARGUMENT, "last hidden layer width %d unsupported by the output-gradient kernel (multiple of 4, <= 960)", Hl);
    if (!l0_mfma_shape(d, n) && l0_seg_shape(d->L[1], l0_chunk_of(n)).lds > 64 * 1024)
        return fail(XQ_ERR_INVALID_ARGUMENT, "first hidden layer too wide for the layer-0 gradient kernel (%d)", d->L[1]);
    size_t need = 0;
    auto place = [&](int nslabs, size_t len) {
        const size_t floats = nslabs > 1 ? (size_t)nslabs * len : 0, at = defer ? need : 0;
        need = defer ? need + floats : std::max(need, floats);
        return at;
    };
    P->off_out = place(P->out_chunks, (size_t)P->len_out);
    for (int l = d->nl - 2; l >= 1; --l) P->off_h[l] = place(grad_splits(d, d->L[l + 1], d->L[l], n), (size_t)d->L[l + 1] * (size_t)d->L[l]);
    XQ_TRY(d->slabs.reserve(need));
    d->pend_w0 = d->pend_wout = d->pend_bout = d->pend_bh = xq_dqn::PendingSlab();
    for (auto& p : d->pend_hidden) p = xq_dqn::PendingSlab();
    return XQ_OK;
}

// output layer rows 0..95 + their biases (g_bout follows g_wout directly): segmented sums by action
static int out_gradient(xq_dqn* d, const GradPlan& P, int n, const float* alast, float* G) {
    const int Hl = d->hlast(), nchunks = P.out_chunks;
    float* dst = G + d->g_wout;
    float* out = nchunks > 1 ? d->slabs + P.off_out : dst;
    const double fl = 2.0 * n * Hl, by = (double)n * (Hl * 4 + 8) + 4.0 * nchunks * P.len_out;
    if (d->tail_open) {
        TailArgs& T = *d->tail;
        T.og_act = d->act_mb; T.og_dsc = d->dsc; T.og_alast = alast; T.og_n = n; T.og_H = Hl; T.og_chunk = kOutGradChunk; T.og_partial = out;
        T.n_out = 24 * nchunks;
        d->tail_flops += fl; d->tail_bytes += by;
        d->tail_lds = std::max(d->tail_lds, P.out_lds);
    } else {
        ProfScope ps(d, "out_grad_segsum", fl, by);
        hipLaunchKernelGGL(out_grad_kernel, dim3(24, nchunks), dim3(256), P.out_lds, d->cur, d->act_mb, d->dsc, alast, n, Hl, kOutGradChunk, out);
        XQ_HIP(hipGetLastError());
    }
    if (nchunks <= 1) return XQ_OK;
    if (P.defer) {
        d->pend_wout.src = out; d->pend_wout.nslabs = nchunks; d->pend_wout.stride = P.len_out;
        d->pend_bout.src = out + 96LL * Hl; d->pend_bout.nslabs = nchunks; d->pend_bout.stride = P.len_out;
        return XQ_OK;
    }
    return launch_reduce_slabs(d, out, nchunks, P.len_out, dst);      // (len_out <= 96 * 961: under the grid cap, one thread per sum)
}
// weight gradient of hidden layer l >= 1: delta_l^T a_{l-1} (XQ_PRECISION_BF16_FULL: on the bf16 loop where the shape allows)
static int hidden_weight_gradient(xq_dqn* d, const GradPlan& P, int l, int n, float* const* outs, float* G) {
    GemmArgs g; memset(&g, 0, sizeof g);
    g.M = d->L[l + 1]; g.N = d->L[l]; g.K = n;
    g.A = d->deltas[l]; g.lda = d->L[l + 1];
    g.B = outs[l - 1]; g.ldb = d->L[l];
    const bool bf = d->bf16_bwd();
    return grad_gemm<L_MCONTIG>(d, g, G + d->g_wh[l], "gemm_grad_hidden", d->slabs + P.off_h[l], P.defer ? &d->pend_hidden[l] : nullptr,
                                bf ? d->deltas_bf[l].p : nullptr, bf ? d->acts_bf[l - 1].p : nullptr);
}
// the hidden biases: column sums of every hidden delta, in the order of the bias vector
static int hidden_bias_gradients(xq_dqn* d, const GradPlan& P, int n, float* G) {
    BiasJobs bj;
    for (int l = 0; l <= d->nl - 2; ++l) bj.add(d->deltas[l], d->L[l + 1], d->L[l + 1], G + d->g_bh[l]);
    return bias_grads(d, bj, n, P.defer ? &d->pend_bh : nullptr);
}

// the order of the side stream (td_gradients_fork): each gradient as soon as its delta exists
static int side_gradients(xq_dqn* d, const GradPlan& P, int n, float* const* outs, float* G) {
    const int nl = d->nl;
    XQ_TRY(out_gradient(d, P, n, outs[nl - 2], G));
    bool waited = false;
    for (int l = nl - 2; l >= 1; --l) {
        if (l < nl - 2 && !waited) { XQ_HIP(hipStreamWaitEvent(d->cur, d->ev_delta, 0)); waited = true; }   // delta_l, l < top, comes from the GEMMs
        XQ_TRY(hidden_weight_gradient(d, P, l, n, outs, G));
    }
    if (!waited) XQ_HIP(hipStreamWaitEvent(d->cur, d->ev_delta, 0));
    return hidden_bias_gradients(d, P, n, G);
}

// ---- the same gradients as fused launches on the handle's stream (td_tail_kernel): no side stream, no event --------------------
// The assembly of one fused launch: from here until launch() (or the end of the scope, whichever comes first) the launch helpers
// append their blocks to d->tail instead of launching.
struct TailGrid {
    xq_dqn* d;
    explicit TailGrid(xq_dqn* d_) : d(d_) {
        if (!d->tail) d->tail = new TailArgs();
        memset(d->tail, 0, sizeof(TailArgs));
        d->tail_open = true; d->tail_lds = 0; d->tail_flops = d->tail_bytes = 0;
    }
    ~TailGrid() { d->tail_open = false; }
    int launch(bool last, const char* name) {
        d->tail_open = false;
        const TailArgs& T = *d->tail;
        const long long total = (long long)T.n_l0 + T.n_grad + T.n_delta + T.n_out + T.n_colsum + T.n_sel + T.n_l0cold;
        if (total <= 0) return XQ_OK;
        ProfScope ps(d, name, d->tail_flops, d->tail_bytes, true);      // one launch: timed by its own start / stop events
        const auto kern = last ? (T.l0_planes != nullptr ? td_tail_kernel<TAIL_L0 | TAIL_GRAD | TAIL_OUT | TAIL_COLSUM, true>
                                                         : td_tail_kernel<TAIL_L0 | TAIL_GRAD | TAIL_OUT | TAIL_COLSUM>)
                               : (T.n_sel ? td_tail_kernel<TAIL_GRAD | TAIL_DELTA | TAIL_OUT | TAIL_SEL> : td_tail_kernel<TAIL_GRAD | TAIL_DELTA | TAIL_OUT>);
        if (d->tail_lds > 48 * 1024) XQ_TRY(ensure_max_dynamic_lds(kern, 64 * 1024));
        hipExtLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), d->tail_lds, d->cur, ps.start(), ps.stop(), 0, T);
        XQ_HIP(hipGetLastError());
        return XQ_OK;
    }
};
// shapes the fused launches take: fp32 products on 64x64 tiles (what launch_gemm picks for them anyway).  Their partial sums stay
// pending: with fused_apply and no communicator the SGD kernel adds them; otherwise ONE launch reduces all of them into the gradient
// buffer behind the second fused launch (reduce_pending), and a communicator all-reduces that buffer behind it.
static bool tail_eligible(xq_dqn* d, int n) {
    if (!d->td_tail || d->bf16()) return false;
    for (int l = 0; l + 2 < d->nl; ++l)
        if (!d->small_tiles && (long long)((n + 127) / 128) * ((d->L[l + 1] + 127) / 128) >= 512) return false;   // launch_gemm would go 128x128
    return true;
}
// every pending partial-sum slab of the step summed into its place in the gradient buffer, one launch (slab_sum's order)
static int reduce_pending(xq_dqn* d) {
    SegTable t; memset(&t, 0, sizeof t);
    float* G = d->grads_td;
    int k = 0;
    for_td_segments(d, [&](float*, uint16_t*, size_t goff, long long len, xq_dqn::PendingSlab& p) {
        if (p.nslabs > 0) { t.dst[k] = G + goff; t.src[k] = p.src; t.len[k] = len; t.nslabs[k] = p.nslabs; t.stride[k] = p.stride; ++k; }
        p = xq_dqn::PendingSlab();
    });
    if (k == 0) return XQ_OK;
    t.nseg = k; t.reduce_only = 1;
    return sgd_apply(d, t, 0.0);
}
// the order of the fused launches: one per hidden layer below the top one — delta_l from delta_{l+1}, the weight gradient of layer
// l+1 (delta_{l+1}, a_l) beside it, the output-layer sums beside the first — then the layer-0 sums with the bias column sums
static int tail_launches(xq_dqn* d, int n, float* const* outs, float* G, int mode) {
    const int nl = d->nl;
    GradPlan P;
    XQ_TRY(plan_gradients(d, n, true, &P));          // a fused grid cannot be followed by its own ordered sums: every slab stays pending
    // two hidden layers: the one weight-gradient product runs beside the layer-0 sums (L2-bound) rather than beside the delta product
    // (both MFMA-bound, and the select chain's Q head is on the chip at that time): 0.2065 against 0.2086 ms per step of the headline
    // bench; three hidden layers (bench --config 4): no difference, kept beside the delta products
    const bool defer_grad = nl == 3;
    int waiting = -1;
    for (int l = nl - 3; l >= 0; --l) {
        TailGrid grid(d);
        XQ_TRY(hidden_deltas(d, n, d->deltas[l + 1], d->L[l + 2], d->L[l + 2], mode, l, l));
        if (defer_grad) { if (waiting >= 0) XQ_TRY(hidden_weight_gradient(d, P, waiting, n, outs, G)); waiting = l + 1; }
        else XQ_TRY(hidden_weight_gradient(d, P, l + 1, n, outs, G));
        if (l == nl - 3) XQ_TRY(out_gradient(d, P, n, outs[nl - 2], G));
        if (l == 0 && l0_mfma_shape(d, n)) {
            // the selector half-words of the minibatch's boards (operand of the matrix-pipe layer-0 gradient in the NEXT launch): they
            // depend on the boards alone, so their blocks ride at the end of this grid, off the dependency chain
            XQ_TRY(ensure_l0_mfma(d, n));
            TailArgs& T = *d->tail;
            const int chunk0 = l0_chunk_of(n), kpad = (n + chunk0 - 1) / chunk0 * chunk0;
            T.sel_boards = d->gboards; T.sel_n = n; T.sel_kpad = kpad; T.sel_out = d->l0_sel; T.n_sel = kpad / 64;
            T.l0_hot = d->hot(); T.sel_cold_list = d->l0_cold_list; T.sel_cold_cnt = d->l0_cold_cnt;
            d->tail_bytes += (double)n * 48 + 2.0 * l0sel_elems(kpad);
            d->tail_lds = std::max(d->tail_lds, (size_t)64 * 13 * sizeof(uint32_t));
            d->l0_sel_done = true;
        }
        XQ_TRY(grid.launch(false, "td_tail_deltas"));
    }
    // last launch (+ the output-layer sums of a net without a second hidden layer)
    TailGrid grid(d);
    XQ_TRY(l0_gradient(d, n, G + d->g_w0, &d->pend_w0));
    if (waiting >= 0) XQ_TRY(hidden_weight_gradient(d, P, waiting, n, outs, G));
    if (nl < 3) XQ_TRY(out_gradient(d, P, n, outs[nl - 2], G));
    XQ_TRY(hidden_bias_gradients(d, P, n, G));
    return grid.launch(true, "td_tail_l0");
}
static int tail_gradients(xq_dqn* d, int n, float* const* outs, float* G, int mode) {
    int rc = tail_launches(d, n, outs, G, mode);
    if (d->late_gate) {                              // the select chain starts here, beside the exchange — also behind a failed step: a
        // collect that waits for ev_qmax must find this step's record, not the previous one's
        if (hipEventRecord(d->ev_qmax, d->stream) != hipSuccess && rc == XQ_OK) rc = fail(XQ_ERR_RUNTIME, "hipEventRecord failed");
    }
    if (rc == XQ_OK && !d->fused()) {                // (fused_apply, no communicator: the apply kernel adds the slabs)
        rc = reduce_pending(d);
        // data-parallel step: the whole buffer in one collective on the handle's stream, right behind its last producer
        if (rc == XQ_OK && d->comm) {
            ProfScope ps(d, "rccl_allreduce_grads", 0, 4.0 * d->n_grads_td);
            rc = comm_allreduce_on(d->comm, G, d->n_grads_td, d->stream);
        }
    }
    return rc;
}

// ---- one TD step (td_grads_impl): the stages below, in the order the step runs them -----------------------------------------------

// The screen's part of one TD step, decided at the step's top (Screen::plan): screened at all (else qmax_exact), with screen_top2_kernel for
// the widths it is built for (else the persistent tile kernel's CM_TOP2 mode), the parity of the wmax slots, the conversion of the shadow
struct ScreenPlan { bool screened, top2; int parity; ShadowJob shadow; };
// What the stages of one step share: its inputs, and the shapes and views decided once at its top.
struct TdStep {
    const int32_t* action_to; const float* reward; const uint8_t* done; SlotSrc slots; const PerOpts* per;
    const uint32_t* next_boards; const uint8_t* next_player; bool legal;       // the legal-move bootstrap: s', its side to move (by slot)
    float gamma;                 // the discount of this step's target: (float)d->gamma, or gamma^n of an n-step batch
    int n, mode, sel_net, nl, Hl, NO; bool dbl, bf;
    bool big_tiles;              // the max pass's product on 128-row tiles
    int n_partial;               // partial maxima per sample of the max pass's tile kernels
    size_t bias_lds;             // the whole output bias in the persistent column-max kernel's LDS
    ScreenPlan scr;              // the screened max pass, or not
    float* outs[XQ_MAX_LAYERS]; uint16_t* outs_bf[XQ_MAX_LAYERS];        // s on the online net (kept for the backward pass)
    float* touts[XQ_MAX_LAYERS]; uint16_t* touts_bf[XQ_MAX_LAYERS];      // s' on the selecting net
    float* t2outs[XQ_MAX_LAYERS]; uint16_t* t2outs_bf[XQ_MAX_LAYERS];    // s' on the target net (Double DQN)
    const float* view; long long view_ld; int view_kmax;                 // the online weights that carry the output delta down a layer
};

// The screening guard.  The counters queued at one check boundary (guard_queue) are evaluated at the NEXT one (guard_tick, 32 screened
// steps later: the copy finished long ago, the wait returns at once) — the step at which a fallback begins is a function of the step
// count alone, never of how far the host runs ahead of the device.  A decision never counts a step that ran before the end of the last
// hold: the hold marks `seen` stale (rebase), the first screened step behind it queues a copy at once, and at the next check boundary
// that copy becomes `seen` without a decision, in front of the boundary's own copy (guard_queue).
// guard_decide: the rule, on the totals of the copy (no runtime call)
void Screen::guard_decide(const unsigned long long h[2]) {
    const double ds = (double)(guard_samples - seen[0]);
    if (ds > 0 && ((double)(h[0] - seen[1]) > kScreenMaxPairs * ds || (double)(h[1] - seen[2]) > kScreenMaxWhole * ds)) {
        hold = kScreenHoldSteps;
        fallbacks += 1;
        rebase = true;                               // (nothing is pending here: the copy just evaluated was)
    }
    if (ds > 0) {                                    // whole groups per sample over the window, with hysteresis
        const double share = (double)(h[1] - seen[2]) / ds;
        if (share > 0.25) stage_whole = true; else if (share < 0.10) stage_whole = false;
    }
    seen[0] = guard_samples; seen[1] = h[0]; seen[2] = h[1];
}
// at the top of a step that asks for the screened max pass.  *screened: whether this step screens
int Screen::guard_tick(bool* screened) {
    if (guard_pending && !rebase && host_steps % kScreenCheckEvery == 0 && host_steps != guard_queued_at) {
        XQ_HIP(hipEventSynchronize(guard_ev));
        guard_pending = false;
        unsigned long long h[2];
        totals_of(guard_host, h);
        guard_decide(h);
    }
    *screened = hold == 0;
    if (hold > 0) --hold;
    return XQ_OK;
}
// behind the launches of a screened step: count it and, every kScreenCheckEvery steps, queue the copy of the counters.  While `rebase`
// is set every copy is a re-basing one: queued behind the first screened step that finds none pending (the first behind the hold, or
// behind a growth of the array that dropped it), taken as `seen` at the next boundary
int Screen::guard_queue(int n, hipStream_t s) {
    host_steps += 1; host_samples += (unsigned long long)n;
    const bool boundary = host_steps % kScreenCheckEvery == 0;
    if (rebase && guard_pending && boundary) {
        XQ_HIP(hipEventSynchronize(guard_ev));
        guard_pending = false; rebase = false;
        unsigned long long h[2];
        totals_of(guard_host, h);
        seen[0] = guard_samples; seen[1] = h[0]; seen[2] = h[1];
    }
    if ((boundary || rebase) && !guard_pending) {
        XQ_HIP(hipMemcpyAsync(guard_host, stats, (size_t)2 * stat_blocks * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        XQ_HIP(hipEventRecord(guard_ev, s));
        guard_pending = true; guard_samples = host_samples; guard_queued_at = host_steps;
    }
    return XQ_OK;
}

// bf16 copy + largest row norm / |bias| of the selecting net's output-layer weights.  Only rows 0..95 change under the TD rule: while
// `static_net` says that rows >= 96 of the shadow (and their maxima, slots [4], [5]) still belong to this net, the shadow pass converts
// three blocks of 32 rows instead of 254; everything is converted again after a write of any other row (params_written) or a change of
// the selecting net.  The maxima of rows 0..95 land in the slots of this step's parity, which the previous screened step's refine kernel zeroed.
int Screen::shadow_job(const xq_dqn* d, int sel_net, int parity, hipStream_t s, ShadowJob* shadow) {
    const int NO = d->nout(), nl = d->nl;
    const bool full = static_net != sel_net;
    if (full) XQ_HIP(hipMemsetAsync(wmax + 4, 0, 2 * sizeof(unsigned), s));     // (the maxima of rows >= 96 start again)
    memset(shadow, 0, sizeof *shadow);
    shadow->W = d->wl(sel_net, nl - 1); shadow->bias = d->bl(sel_net, nl - 1); shadow->NO = NO; shadow->K = d->hlast(); shadow->Wb = wb;
    shadow->w_dyn = wmax + parity; shadow->b_dyn = wmax + 2 + parity;
    shadow->w_stat = wmax + 4; shadow->b_stat = wmax + 5;
    shadow->nblocks = full ? (NO + kShadowRows - 1) / kShadowRows : std::min((int)kShadowDynBlocks, (NO + kShadowRows - 1) / kShadowRows);
    static_net = sel_net;
    return XQ_OK;
}

// This step's part of the screen: the eligibility of its shape, the guard, the parity of its slots and the shadow conversion
int Screen::plan(xq_dqn* d, const TdStep& s, ScreenPlan* P) {
    const bool want_screen = mode == XQ_QMAX_SCREENED && !s.legal && !s.bf && !s.dbl && s.big_tiles && (s.Hl % 64) == 0 && s.Hl <= 1024 &&
                             s.bias_lds <= 40 * 1024 && (s.NO + 127) / 128 * 4 <= 8 * kRefineMaxPerThread;
    P->screened = false;
    if (want_screen) {
        XQ_TRY(reserve(s.NO, s.Hl, s.n, d->params[0].p, d->tacts[0].p));
        XQ_TRY(guard_tick(&P->screened));
    }
    P->parity = (int)(host_steps & 1);
    P->top2 = P->screened && (s.Hl == 256 || s.Hl == 512);
    if (P->screened) XQ_TRY(shadow_job(d, s.sel_net, P->parity, d->cur, &P->shadow));
    return XQ_OK;
}

// screen_top2_kernel (xq_screen.hip.h) in mode SCR_TOP2 / SCR_ARG / SCR_MAX for a 256- or 512-wide last hidden layer
static int launch_screen(xq_dqn* d, const ScreenArgs& a, int mode, hipEvent_t start, hipEvent_t stop) {
    using ScreenKernel = void (*)(ScreenArgs);
    static const ScreenKernel kerns[3][2] = {{screen_top2_kernel<1, 2, SCR_TOP2>, screen_top2_kernel<2, 1, SCR_TOP2>},
                                             {screen_top2_kernel<1, 2, SCR_ARG>, screen_top2_kernel<2, 1, SCR_ARG>},
                                             {screen_top2_kernel<1, 2, SCR_MAX>, screen_top2_kernel<2, 1, SCR_MAX>}};
    const ScreenKernel kern = kerns[mode][a.K == 256 ? 0 : 1];
    XQ_TRY(ensure_max_dynamic_lds(kern, 160 * 1024));
    hipExtLaunchKernelGGL(kern, dim3(a.panels * a.ranges), dim3(512), screen_lds_bytes(a), d->cur, start, stop, 0, a);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// gemm_colmax_persistent_kernel (xq_gemm.hip.h) over `total` tiles of 128 x 128: 2 blocks per CU walk the tile list with the prefetch
// running across tile boundaries, the second half of the grid its own half of the tiles at static priority (see the kernel).  Sets the
// walk's fields of g (zeroed, with g.M, g.K and g.bias set) and returns the grid.
static int colmax_persistent_grid(const xq_dqn* d, GemmArgs& g, int tiles_m, int total) {
    g.a_vec = g.b_vec = 1; g.k_chunk = g.K;
    g.bias_padded = ((((uintptr_t)g.bias) % 16 == 0) && (g.M % 4) == 0) ? 1 : 0;     // wide bias preload
    const int grid = std::min(total, 2 * d->ncu);
    if (grid >= 2 && (grid & 1) == 0 && total >= 4 * grid) {
        g.prio_split = grid / 2;
        g.prio_tiles = (total / 2) / tiles_m * tiles_m;
        if (g.prio_tiles <= 0 || g.prio_tiles >= total) { g.prio_split = 0; g.prio_tiles = 0; }
    }
    return grid;
}

// Screened max_a' Q(s', a') of an fp32 net: the bf16 screening product (screen_top2_kernel for the widths it is built for,
// the persistent tile kernel's CM_TOP2 mode otherwise), the exact fp32 refine of the candidates it leaves, and the guard's count of the step
// (Screen::guard_queue).  *td_fused: the refine kernel did td_delta_kernel's work too.
static int qmax_screened(xq_dqn* d, const TdStep& s, bool* td_fused) {
    const int n = s.n, NO = s.NO, Hl = s.Hl, nl = s.nl, parity = s.scr.parity;
    const bool top2 = s.scr.top2;  Screen& scr = d->scr;
    const float *W = d->wl(s.sel_net, nl - 1), *bias = d->bl(s.sel_net, nl - 1);
    const int tiles_m = (NO + 127) / 128, total = tiles_m * ((n + 127) / 128);
    // 32-row lane groups: the tile kernel writes all 4 per 128-row tile, screen_top2_kernel only those of 64-row chunks with real rows
    const int G = top2 ? 2 * ((NO + 63) / 64) : 4 * tiles_m;
    long long ldp = n;
    int ranges = 0, gpr = 0;
    if (top2) {
        ScreenArgs a; memset(&a, 0, sizeof a);
        a.W = scr.wb; a.A = scr.ab; a.a_frag = 1; a.bias = bias;
        a.P1 = scr.p1; a.P2 = scr.p2; a.R = scr.R; a.na = scr.na;
        screen_geometry(NO, n, Hl, d->ncu, a);
        ldp = a.ldp = screen_padded_samples(n, Hl);
        ranges = a.ranges; gpr = 2 * a.cpr;
        // (bracketed by its own start / stop events: the live figure is the kernel's duration as rocprofv3 reports it)
        ProfScope ps(d, "gemm_qmax_screen", 2.0 * NO * (double)n * Hl, 2.0 * ((double)NO * Hl + (double)n * Hl) + 8.0 * G * n, true);
        XQ_TRY(launch_screen(d, a, SCR_TOP2, ps.start(), ps.stop()));
    } else {
        GemmArgs g; memset(&g, 0, sizeof g);
        g.M = NO; g.N = n;
        g.K = Hl / 2; g.lda = g.ldb = Hl / 2;
        g.A = reinterpret_cast<const float*>(scr.wb.p); g.B = reinterpret_cast<const float*>(scr.ab.p);
        g.bias = bias;
        g.partial = scr.p1; g.partial2 = scr.p2;
        const int grid = colmax_persistent_grid(d, g, tiles_m, total);
        ProfScope ps(d, "gemm_qmax_screen", 2.0 * g.M * g.N * Hl, 2.0 * ((double)g.M * Hl + (double)g.N * Hl) + 8.0 * G * g.N);
        hipLaunchKernelGGL((gemm_colmax_persistent_kernel<2, 2, DT_BF16, CM_TOP2>), dim3(grid), dim3(256), s.bias_lds, d->cur, g, tiles_m, total);
        XQ_HIP(hipGetLastError());
    }
    // (the select chain of the trainer started in front of the screening pass.  Behind the refine kernel instead — which would then have
    // the chip to itself, 17 instead of 27-34 us — the select chain ends after the gradients and the step waits for it: 0.197 -> 0.207 ms)
    {
        ProfScope ps(d, "qmax_refine", 2.0 * n * Hl * 3, 12.0 * G * n + 4.0 * n * Hl, true);      // one launch: its own start / stop events
        const dim3 grid((n + kRefineSamples - 1) / kRefineSamples);
        // one block per CU and K = 256: room in LDS for the staged pass of qmax_refine2_kernel (whole groups that many samples ask for)
        const bool stage = top2 && Hl == 256 && (int)grid.x <= d->ncu && (scr.refine_stage > 0 || (scr.refine_stage < 0 && scr.stage_whole));
        const size_t lds = refine_cand_words(G) * sizeof(uint32_t) + refine_wlist_bytes(G) + (stage ? refine_stage_bytes() : 0);
        const float* a_last = s.touts[nl - 2];
        if (top2) {
            TdFused T; memset(&T, 0, sizeof T);
            // the TD target / delta kernel rides in the refine blocks (fp32 net, 256-wide last hidden layer, uniform replay)
            *td_fused = d->td_tail && Hl == 256 && !s.per && !d->bf16_bwd();
            if (*td_fused) {
                const int lt = nl - 2;
                T.src = s.slots; T.action_to = s.action_to; T.reward = s.reward; T.done = s.done;
                T.a_s = s.outs[lt]; T.w_out = d->wl(XQ_NET_ONLINE, nl - 1); T.b_out = d->bl(XQ_NET_ONLINE, nl - 1);
                T.view = s.view; T.view_ld = s.view_ld; T.view_kmax = s.view_kmax; T.gamma = s.gamma;
                T.dtop = d->deltas[lt]; T.dsc = d->dsc; T.act = d->act_mb; T.qsa = d->qsa; T.yv = d->yv; T.lossv = d->lossv;
            }
            // whole groups: 2 = the popular ones through LDS when the launch has room for it, 1 = all of them four per round trip
            const int whole_mode = stage ? 2 : 1;
            const auto launch = [&](auto kern, auto loss) -> int {        // the one launch of the family; the loss is its last argument
                XQ_TRY(ensure_max_dynamic_lds(kern, 152 * 1024));          // the staged pass asks for ~145 KB
                hipExtLaunchKernelGGL(kern, grid, dim3(256), lds, d->cur, ps.start(), ps.stop(), 0, scr.R.p, ranges, gpr, scr.p1.p, scr.p2.p,
                                      G, n, ldp, scr.na.p, a_last, Hl, W, bias, NO, scr.wmax.p, parity, d->zmax.p, scr.stats.p, T, whole_mode, loss);
                return XQ_OK;
            };
            if (*td_fused && d->loss_kind == XQ_LOSS_HUBER) XQ_TRY(launch(qmax_refine2_kernel<256, true, HuberLoss>, HuberLoss{d->loss_kappa32}));
            else XQ_TRY(launch(*td_fused ? qmax_refine2_kernel<256, true> : Hl == 256 ? qmax_refine2_kernel<256> : qmax_refine2_kernel<512>, SquaredLoss{}));
        } else {
            const bool small = G <= 8 * 32;
            const auto kern = Hl == 256 ? (small ? qmax_refine_kernel<256, 32> : qmax_refine_kernel<256, 64>)
                            : Hl == 512 ? (small ? qmax_refine_kernel<512, 32> : qmax_refine_kernel<512, 64>)
                                        : (small ? qmax_refine_kernel<0, 32> : qmax_refine_kernel<0, 64>);
            hipExtLaunchKernelGGL(kern, grid, dim3(256), lds, d->cur, ps.start(), ps.stop(), 0, scr.p1.p, scr.p2.p, G, n, ldp, a_last, Hl,
                                  W, bias, NO, scr.wmax.p, parity, d->zmax.p, scr.stats.p);
        }
        XQ_HIP(hipGetLastError());
    }
    return scr.guard_queue(n, d->cur);
}

// Exact max_a' Q(s', a') (+ its row for Double DQN): partial maxima per sample from one of three products — the screen kernel's exact
// mode (bf16 net), the persistent column-max kernel, launch_gemm's column-max epilogue — folded into kReduceParts values by colmax_reduce.
static int qmax_exact(xq_dqn* d, const TdStep& s, bool bf_frag, bool gate_early) {
    const int n = s.n, NO = s.NO, Hl = s.Hl, nl = s.nl;
    const bool bf = s.bf, dbl = s.dbl;
    long long part_ld = n;              // row stride of the partial arrays
    int n_part = s.n_partial;
    if (bf && (Hl == 256 || Hl == 512) && n >= 1024) {
        // bf16 Q-net: the same kernel as the screening pass in its exact max / arg-max mode — here the bf16 product IS the net's output
        // layer, not a screen: per 32-row lane group the largest value (+ its row, first maximum: Double DQN)
        ScreenArgs a; memset(&a, 0, sizeof a);
        a.W = d->wl_bf(s.sel_net, nl - 1); a.A = s.touts_bf[nl - 2]; a.a_frag = bf_frag ? 1 : 0; a.bias = d->bl(s.sel_net, nl - 1);
        a.P1 = d->partial; a.P2 = reinterpret_cast<float*>(d->partial_idx.p);
        screen_geometry(NO, n, Hl, d->ncu, a);
        part_ld = a.ldp = screen_padded_samples(n, Hl);
        n_part = 2 * a.nchunks;
        ProfScope ps(d, "gemm_qmax_rowmax", 2.0 * NO * (double)n * Hl, 2.0 * ((double)NO * Hl + (double)n * Hl) + 8.0 * n_part * n, true);
        XQ_TRY(launch_screen(d, a, dbl ? SCR_ARG : SCR_MAX, ps.start(), ps.stop()));
    } else {
        GemmArgs g; memset(&g, 0, sizeof g);
        g.M = NO; g.N = n;
        g.K = bf ? Hl / 2 : Hl; g.lda = g.ldb = g.K;        // (bf16 operands: pairs of elements as one fp32 word)
        g.A = bf ? reinterpret_cast<const float*>(d->wl_bf(s.sel_net, nl - 1)) : d->wl(s.sel_net, nl - 1);
        g.B = bf ? reinterpret_cast<const float*>(s.touts_bf[nl - 2]) : s.touts[nl - 2];
        g.bias = d->bl(s.sel_net, nl - 1);
        g.partial = d->partial;
        g.partial_idx = dbl ? d->partial_idx : nullptr;
        // the persistent kernel keeps the whole bias vector in LDS beside its operand tiles (2 blocks per CU must fit)
        if (s.big_tiles && (g.K % GBK) == 0 && vec_ok(g.A, g.lda) && vec_ok(g.B, g.ldb) && s.bias_lds <= 40 * 1024) {
            const int tiles_m = (NO + 127) / 128, total = tiles_m * ((n + 127) / 128);
            const int grid = colmax_persistent_grid(d, g, tiles_m, total);
            ProfScope ps(d, "gemm_qmax_rowmax", 2.0 * g.M * g.N * Hl, (bf ? 2.0 : 4.0) * ((double)g.M * Hl + (double)g.N * Hl) + 8.0 * tiles_m * g.N);
            const auto kern = bf ? (dbl ? gemm_colmax_persistent_kernel<2, 2, DT_BF16, CM_ARG> : gemm_colmax_persistent_kernel<2, 2, DT_BF16, CM_MAX>)
                                 : (dbl ? gemm_colmax_persistent_kernel<2, 2, DT_F32, CM_ARG> : gemm_colmax_persistent_kernel<2, 2, DT_F32, CM_MAX>);
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), s.bias_lds, d->cur, g, tiles_m, total);
            XQ_HIP(hipGetLastError());
        } else if (bf) XQ_TRY((launch_gemm<L_KCONTIG, L_KCONTIG, EPI_COLMAX, DT_BF16>(d, g, 1, "gemm_qmax_rowmax")));
        else XQ_TRY((launch_gemm<L_KCONTIG, L_KCONTIG, EPI_COLMAX>(d, g, 1, "gemm_qmax_rowmax")));
    }
    if (!d->late_gate && !gate_early) XQ_HIP(hipEventRecord(d->ev_qmax, d->stream));
    {   // the partial maxima of every sample folded into kReduceParts values (+ row indices): coalesced, block-cooperative
        ProfScope ps(d, "colmax_reduce", (double)n * n_part, (dbl ? 8.0 : 4.0) * n * (n_part + kReduceParts));
        hipLaunchKernelGGL(colmax_reduce_kernel, dim3((n + 63) / 64, kReduceParts), dim3(256), 0, d->cur, d->partial,
                           dbl ? d->partial_idx : nullptr, n_part, n, part_ld, d->zmax, d->zidx);
        XQ_HIP(hipGetLastError());
    }
    return XQ_OK;
}

// Legal-move bootstrap (xq_dqn_set_td_bootstrap): the 96-row head product of s' on the selecting net as k-slabs (q_head's
// split: four blocks per CU instead of one walking all of K) and legal_qmax_kernel, which sums them, generates the moves of the side to
// move in s' and leaves in zmax the pre-activation of the env kernel's greedy pick.  Double DQN: the same product on the target net's s'
// chain as well; the kernel picks on the online values and leaves the target net's value of that output, so td_delta runs its one-net
// form (its own Double path has no way to give a row without a move y = r).
static int qmax_legal(xq_dqn* d, const TdStep& s, bool gate_early) {
    const int n = s.n, nl = s.nl, Hl = s.Hl;
    const int want = (n >= 2048 && (Hl % 128) == 0) ? std::min(Hl / 64, (int)kLegalMaxSlabs) : 1;
    const int nets = s.dbl ? 2 : 1;
    const long long slab_stride = (long long)n * 96;
    XQ_TRY(d->z96_slabs.reserve((size_t)nets * want * slab_stride));
    XQ_TRY(d->z96.reserve((size_t)slab_stride));
    XQ_TRY(d->legal_nmoves.reserve((size_t)n));
    int used[2] = {want, want};
    for (int k = 0; k < nets; ++k) {
        GemmArgs g; memset(&g, 0, sizeof g);
        g.M = n; g.N = 96; g.K = Hl;
        g.A = k == 0 ? s.touts[nl - 2] : s.t2outs[nl - 2]; g.lda = Hl;
        g.B = d->wl(k == 0 ? s.sel_net : XQ_NET_TARGET, nl - 1); g.ldb = Hl;
        g.C = d->z96_slabs + (size_t)k * want * slab_stride; g.ldc = 96; g.slab_stride = slab_stride;
        XQ_TRY((launch_gemm<L_KCONTIG, L_KCONTIG, EPI_STORE>(d, g, want, "gemm_legal_head", &used[k], true)));
    }
    if (used[0] < 1 || used[0] > want || (s.dbl && used[1] != used[0])) return fail(XQ_ERR_RUNTIME, "legal head: %d k-slabs for %d asked", used[0], want);
    LegalArgs A; memset(&A, 0, sizeof A);
    A.next_boards = s.next_boards; A.action_to = s.action_to; A.done = s.done; A.side = s.next_player;
    A.sel_slabs = d->z96_slabs; A.sel_bias = d->bl(s.sel_net, nl - 1);
    if (s.dbl) { A.ev_slabs = d->z96_slabs + (size_t)want * slab_stride; A.ev_bias = d->bl(XQ_NET_TARGET, nl - 1); }
    A.slab_stride = slab_stride; A.nslabs = used[0];
    A.z96 = d->z96; A.zmax = d->zmax; A.zidx = d->zidx; A.n_moves = d->legal_nmoves;
    A.no_move_zmax = d->zero_sum ? -__builtin_inff() : 0.f;      // zero-sum: a side that cannot move has lost, y = r + g
    // per row: the board, 6 B of fields, nets x nslabs x 96 slab values in, 96 values and 12 B out
    ProfScope ps(d, "legal_qmax", 0.0, (double)n * (48 + 6 + 384.0 * nets * used[0] + 384 + 12), true);
    hipExtLaunchKernelGGL(legal_qmax_kernel, dim3((n + 3) / 4), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, A, s.slots, n);
    XQ_HIP(hipGetLastError());
    if (!d->late_gate && !gate_early) XQ_HIP(hipEventRecord(d->ev_qmax, d->stream));    // (not reached: a legal step gates early)
    return XQ_OK;
}

// Q(s, a), target, the scalar output delta and the delta of the last hidden layer (one launch, no GEMM); zparts = maxima per sample in zmax
static int td_delta(xq_dqn* d, const TdStep& s, int zparts) {
    const int n = s.n, nl = s.nl, Hl = s.Hl;
    const int lt = nl - 2;                                   // last hidden layer
    ProfScope ps(d, "td_target_delta", 4.0 * n * Hl, (double)n * (Hl * 16 + s.n_partial * 4));
    TdExtra X; memset(&X, 0, sizeof X);
    X.nout = s.NO;
    if (s.dbl && !s.legal) {             // (legal bootstrap: zmax already holds the target net's value of the online pick)
        X.double_dqn = 1; X.partial_idx = d->zidx;
        X.bout_t = d->bl(XQ_NET_TARGET, nl - 1);
        if (s.bf) { X.wout_t_bf = d->wl_bf(XQ_NET_TARGET, nl - 1); X.alast_t_bf = s.t2outs_bf[lt]; }
        else { X.wout_t = d->wl(XQ_NET_TARGET, nl - 1); X.alast_t = s.t2outs[lt]; }
    }
    if (s.bf) X.wout_bf = d->wl_bf(XQ_NET_ONLINE, nl - 1);
    if (d->bf16_bwd()) X.dtop_bf = d->deltas_bf[lt];
    if (const PerOpts* per = s.per) {
        X.is_w = per->is_w; X.is_wmax = per->is_wmax; X.prio = per->prio; X.pmax_live = per->pmax_live;
        X.per_eps = per->eps; X.per_alpha = per->alpha;
    }
    const auto launch = [&](auto kern, auto... loss) {                  // the one launch of the family; what the loss adds goes last
        hipLaunchKernelGGL(kern, dim3((n + 3) / 4), dim3(256), 0, d->cur, n, s.slots, s.action_to, s.reward, s.done,
                           s.outs[lt], Hl, d->wl(XQ_NET_ONLINE, nl - 1), d->bl(XQ_NET_ONLINE, nl - 1), d->zmax, zparts,
                           s.gamma, s.view, s.view_ld, s.view_kmax, d->deltas[lt], d->dsc, d->act_mb, d->qsa, d->yv, d->lossv, X, loss...);
    };
    if (d->loss_kind == XQ_LOSS_HUBER) launch(td_delta_huber_kernel, d->loss_kappa32);
    else launch(td_delta_kernel);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// The gradients outside the fused launches, two chains side by side.  Critical (handle stream): the remaining hidden deltas and the layer-0
// sums that consume delta_0.  Side stream: the output-layer and hidden weight gradients and the bias column sums, as their deltas exist.
static int td_gradients_fork(xq_dqn* d, const TdStep& s) {
    const int n = s.n, nl = s.nl;
    float* G = d->grads_td;
    GradPlan P;
    XQ_TRY(plan_gradients(d, n, d->fused(), &P));
    xq_dqn::PendingSlab* defer_w0 = P.defer ? &d->pend_w0 : nullptr;
    XQ_HIP(hipEventRecord(d->ev_fork, d->stream));
    XQ_HIP(hipStreamWaitEvent(d->side, d->ev_fork, 0));
    if (nl >= 3) XQ_TRY(hidden_deltas(d, n, d->deltas[nl - 2], d->L[nl - 1], d->L[nl - 1], s.mode, nl - 3));
    XQ_HIP(hipEventRecord(d->ev_delta, d->stream));
    // data-parallel step: the gradient buffer is all-reduced in two buckets, each ON THE STREAM OF ITS PRODUCER right behind it — no
    // communicator stream, no event of its own.  RCCL runs the collectives of one communicator in issue order, so the side bucket (hidden +
    // output-layer weights, all biases: ready first) is issued first and the layer-0 bucket (the last thing computed, the only exposed one)
    // second; every rank issues in this order.  Without a communicator the layer-0 sums are issued first.
    const size_t n0 = (size_t)d->L[0] * d->L[1];
    if (!d->comm) XQ_TRY(l0_gradient(d, n, G + d->g_w0, defer_w0));
    {
        OnStream side(d, d->side);
        XQ_TRY(side_gradients(d, P, n, s.outs, G));
    }
    if (d->comm) XQ_TRY(comm_allreduce_on(d->comm, G + n0, d->n_grads_td - n0, d->side));
    XQ_HIP(hipEventRecord(d->ev_join, d->side));
    if (d->comm) {
        XQ_TRY(l0_gradient(d, n, G + d->g_w0, defer_w0));
        XQ_TRY(comm_allreduce_on(d->comm, G, n0, d->stream));
    }
    XQ_HIP(hipStreamWaitEvent(d->stream, d->ev_join, 0));
    return XQ_OK;
}

static int td_grads_impl(xq_dqn* d, const uint32_t* boards, const uint32_t* next_boards, const int32_t* action_to,
                         const float* reward, const uint8_t* done, SlotSrc slots, int n, int td_net, int mode, const PerOpts* per,
                         const float* discount, const uint8_t* next_player) {
    if (!d || !boards || !next_boards || !action_to || !reward || !done || n <= 0)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_td_grads: bad argument");
    if (td_net != XQ_TD_ONLINE_NET && td_net != XQ_TD_TARGET_NET && td_net != XQ_TD_DOUBLE) return fail(XQ_ERR_INVALID_ARGUMENT, "bad td_net");
    if (mode != XQ_BACKPROP_REFERENCE && mode != XQ_BACKPROP_TEXTBOOK) return fail(XQ_ERR_INVALID_ARGUMENT, "bad backprop mode");
    if (d->nout() < 96) return fail(XQ_ERR_INVALID_ARGUMENT, "TD path needs >= 96 outputs (action.to indexes outputs 0..89)");
    if (mode == XQ_BACKPROP_REFERENCE) XQ_TRY(check_reference_topology(d));
    const bool dbl = td_net == XQ_TD_DOUBLE, bf = d->bf16();
    const bool legal = d->bootstrap == XQ_BOOTSTRAP_LEGAL;
    if (legal && bf) return fail(XQ_ERR_INVALID_ARGUMENT, "the legal-move bootstrap needs an fp32 net (xq_dqn_set_precision)");
    if (legal && !next_player)
        return fail(XQ_ERR_INVALID_ARGUMENT, "the legal-move bootstrap needs the side to move in s': use xq_dqn_td_grads_sided / xq_dqn_td_update_host_sided");
    d->legal_rows = 0;
    d->l0_split_done = d->l0_sel_done = false;       // (set by this step's launches, consumed by l0_gradient)
    // Data-parallel step with more than one rank: the trainer's select chain (it waits for ev_qmax) starts behind the GRADIENTS
    // instead of behind the max pass, so that it runs beside the all-reduce — the exchange is then hidden behind work the step has to
    // do anyway, and the gradient kernels have the chip to themselves.  On one GPU there is nothing to hide behind and the early start
    // is the faster one.
    d->late_gate = d->comm != nullptr && tail_eligible(d, n) &&
                   (d->exchange_overlap == 1 ||
                    (d->exchange_overlap < 0 && (d->exch_calibrated ? d->exch_late : comm_world(d->comm) > 1)));
    XQ_TRY(ensure_capacity(d, n));
    XQ_TRY(ensure_ext_capacity(d, n, dbl));
    const int nl = d->nl, Hl = d->hlast(), NO = d->nout();
    if (bf && (Hl & 1)) return fail(XQ_ERR_INVALID_ARGUMENT, "bf16 Q-net needs even layer widths");
    TdStep s;
    s.action_to = action_to; s.reward = reward; s.done = done; s.slots = slots; s.per = per;
    s.next_boards = next_boards; s.next_player = next_player; s.legal = legal;
    // zero-sum: the signed discount -g (r + (-g) t and r - g t are the same fp32 bits, contracted or not); an n-step batch's discount
    // comes signed from nstep_assemble
    s.gamma = discount ? *discount : d->zero_sum ? -(float)d->gamma : (float)d->gamma;
    d->staged.last = {};                             // (td_grads_ring_staged sets it behind a step on the staging batch)
    s.n = n; s.mode = mode; s.nl = nl; s.Hl = Hl; s.NO = NO; s.dbl = dbl; s.bf = bf; s.sel_net = td_net == XQ_TD_TARGET_NET ? XQ_NET_TARGET : XQ_NET_ONLINE;
    chain_views(d, d->acts, d->acts_bf, XQ_MAX_LAYERS, true, s.outs, s.outs_bf);
    chain_views(d, d->tacts, d->tacts_bf, 2, !bf, s.touts, s.touts_bf);
    chain_views(d, d->t2acts, d->t2acts_bf, 2, !bf, s.t2outs, s.t2outs_bf);
    // the max pass is launched transposed (rows = output neurons, columns = samples): the max over the 8100 outputs then runs over
    // accumulator registers inside one lane instead of across the 32 lanes of a row
    s.big_tiles = (long long)((NO + 127) / 128) * ((n + 127) / 128) >= 512;
    s.n_partial = 2 * (s.big_tiles ? (NO + 127) / 128 : (NO + 63) / 64);
    s.bias_lds = (size_t)((NO + 127) / 128) * 128 * sizeof(float);
    s.view = d->wrest(XQ_NET_ONLINE) + (d->wo[nl - 1] - d->wo[1]);
    s.view_ld = mode == XQ_BACKPROP_REFERENCE ? d->L[nl - 2] : d->L[nl - 1]; s.view_kmax = mode == XQ_BACKPROP_REFERENCE ? d->L[nl - 1] : NO;
    XQ_TRY(d->scr.plan(d, s, &s.scr));
    const bool screened = s.scr.screened;
    // 1. the forward chains in the same launches (one gather grid, grouped hidden GEMMs): s on the online net with the activations kept
    //    for the backward pass, s' on the net that selects (online, or target for XQ_TD_TARGET_NET) and, for Double DQN, s' on the target
    //    net that evaluates.  bf16 net: the s' chain's last activations feed only the max / arg-max pass; when both that pass and the
    //    forward product run on their own loops (whole tiles), the product writes them in fragment order
    const bool bf_frag = bf && nl >= 3 && (Hl == 256 || Hl == 512) && n >= 1024 && (n % kBgBM) == 0 && (d->L[nl - 2] % kBgBK) == 0;
    ChainJob jobs[3] = {{XQ_NET_ONLINE, boards, s.outs, s.outs_bf, d->gboards, nullptr, false},
                        {s.sel_net, next_boards, s.touts, s.touts_bf, nullptr, screened ? d->scr.ab : nullptr, s.scr.top2 || bf_frag},
                        {XQ_NET_TARGET, next_boards, s.t2outs, s.t2outs_bf, nullptr, nullptr, false}};
    // The select chain of the trainer starts at the end of the forward product (its stop event, when chain_boards can take it) when
    // max_a' Q(s',a') runs on the bf16 matrix pipe (screening pass of an fp32 net, or the output layer of a bf16 net): its layer-0 gather
    // (L2-bound) then runs beside the screening pass (matrix-pipe-bound) and is gone when the refine kernel — a chain of dependent memory
    // round trips that the gather doubles in length — starts.  Same-box A/B, round 4 (3 x 300 steps per leg): behind the screening pass
    // 0.1946-0.1969 ms, here 0.1888-0.1937; behind the layer-0 gather of this step 0.1886-0.1896 against 0.1914-0.1921; at the very top of
    // the step no difference; --config 4 / 5 -0.3 % / -0.9 %.  The product's stop event rather than a marker behind it: 0.1740 -> 0.1728 ms.
    // The full fp32 product keeps the chip to itself: there the chain starts behind it (qmax_exact).
    // A legal step starts it there too: behind legal_qmax_kernel the chain ran beside the fused gradient launches and the step came out
    // slower than the screened one (0.169-0.176 against 0.163-0.165 ms through the trainer, profiles/NOTES.md "Legal-move bootstrap").  What
    // runs behind the early gate reads ring slots (legal_qmax_kernel, td_delta) exactly as the refine kernel with the TD delta inside does:
    // the trainer's collect writes only slots its windowed draw left out.
    const bool gate_early = (screened || bf || legal) && !d->late_gate;
    hipEvent_t fork = gate_early ? d->ev_qmax : nullptr;
    XQ_TRY(chain_boards(d, jobs, dbl ? 3 : 2, slots, n, screened ? &s.scr.shadow : nullptr, &fork));
    if (fork) XQ_HIP(hipEventRecord(fork, d->stream));             // chain_boards did not take the stop event: a marker instead
    // 2. max_a' Q(s', a'); 3. the TD delta, unless the refine kernel did it
    bool td_fused = false;
    if (legal) XQ_TRY(qmax_legal(d, s, gate_early));
    else if (screened) XQ_TRY(qmax_screened(d, s, &td_fused));
    else XQ_TRY(qmax_exact(d, s, bf_frag, gate_early));
    if (!td_fused) XQ_TRY(td_delta(d, s, legal || screened ? 1 : kReduceParts));
    d->last_n = n;
    if (legal) d->legal_rows = n;
    // 4. the gradients
    if (tail_eligible(d, n)) return tail_gradients(d, n, s.outs, d->grads_td, mode);
    return td_gradients_fork(d, s);
}

// The late start of the select chain (beside the all-reduce instead of beside the gradient kernels) costs a step ~41 us when the
// collective is free and wins by the part of the collective above that (0.2430 against 0.2021 ms with a one-rank
// communicator, where the all-reduce launches nothing).
static const double kExchangeThresholdUs = 41.0;

int xq_dqn_calibrate_exchange(xq_dqn* d, double threshold_us, double* allreduce_us, int* late) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (!d->comm) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_calibrate_exchange: no communicator attached");
    if (d->n_grads_td == 0) layout_td_grads(d);
    // COLLECTIVE: every rank times the same 4 + 20 all-reduces of a scratch buffer of the gradient buffer's size on the handle's stream
    DevBuf<float> scratch;
    XQ_TRY(scratch.alloc(d->n_grads_td));
    float ms = 0.f;
    const int reps = 20;
    {
        struct SyncOnExit {                          // nothing queued reads the scratch buffer when it goes, however this returns
            hipStream_t s;
            ~SyncOnExit() { (void)hipStreamSynchronize(s); }
        } drained{d->stream};
        Event e0, e1;
        XQ_HIP(hipMemsetAsync(scratch, 0, d->n_grads_td * sizeof(float), d->stream));
        XQ_TRY(e0.create(hipEventDefault));
        XQ_TRY(e1.create(hipEventDefault));
        for (int i = 0; i < 4; ++i) XQ_TRY(comm_allreduce_on(d->comm, scratch, d->n_grads_td, d->stream));
        XQ_HIP(hipEventRecord(e0, d->stream));
        for (int i = 0; i < reps; ++i) XQ_TRY(comm_allreduce_on(d->comm, scratch, d->n_grads_td, d->stream));
        XQ_HIP(hipEventRecord(e1, d->stream));
        XQ_HIP(hipEventSynchronize(e1));
        XQ_HIP(hipEventElapsedTime(&ms, e0, e1));
    }
    // the ranks must agree (a rank that starts its select chain late while its neighbours start early only wastes what the rule
    // saves): the decision is taken on the MEAN over the ranks, in integer nanoseconds so that every rank computes the same number
    uint64_t ns = (uint64_t)((double)ms * 1e6 / reps + 0.5);
    if (ns == 0) ns = 1;                             // (a one-rank all-reduce launches nothing: two back-to-back event records)
    XQ_TRY(xq_comm_sum_u64(d->comm, &ns));
    d->exch_allreduce_us = (double)ns / 1e3 / (double)comm_world(d->comm);
    d->exch_threshold_us = threshold_us >= 0.0 ? threshold_us : kExchangeThresholdUs;
    d->exch_late = d->exch_allreduce_us > d->exch_threshold_us;
    d->exch_calibrated = true;
    if (allreduce_us) *allreduce_us = d->exch_allreduce_us;
    if (late) *late = d->exch_late ? 1 : 0;
    return XQ_OK;
}

int xq_dqn_exchange_calibration(const xq_dqn* d, int* calibrated, double* allreduce_us, double* threshold_us, int* late) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (calibrated) *calibrated = d->exch_calibrated ? 1 : 0;
    if (allreduce_us) *allreduce_us = d->exch_allreduce_us;
    if (threshold_us) *threshold_us = d->exch_threshold_us;
    if (late) *late = d->exch_late ? 1 : 0;
    return XQ_OK;
}

int xq_dqn_set_comm(xq_dqn* d, xq_comm* comm) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (td_step_pending(d))
        return fail(XQ_ERR_RUNTIME, "xq_dqn_set_comm: a TD step is waiting for its apply_grads");
    d->comm = comm;
    d->exch_calibrated = false;
    // more than one rank: measure the exchange now (collective: every rank attaches its communicator at the same point of the program)
    // and let the measurement, not the rank count, say where the select chain starts (the static guess cost 20 % at
    // the one point it had been measured)
    if (comm && comm_world(comm) > 1 && d->exchange_overlap < 0) XQ_TRY(xq_dqn_calibrate_exchange(d, -1.0, nullptr, nullptr));
    return XQ_OK;
}
int xq_allreduce_grads(xq_dqn* d, xq_comm* comm) {
    if (!d || !comm) return fail(XQ_ERR_INVALID_ARGUMENT, "null handle");
    if (td_step_pending(d))
        return fail(XQ_ERR_RUNTIME, "xq_allreduce_grads: gradient slabs are still unreduced (xq_dqn_set_fused_apply is on)");
    return comm_allreduce_on(comm, d->grads_td, d->n_grads_td, d->stream);      // in order on the handle's stream
}

int xq_dqn_apply_grads(xq_dqn* d, double lr, double grad_scale) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    SegTable t; memset(&t, 0, sizeof t);
    const float* G = d->grads_td;
    int k = 0;
    for_td_segments(d, [&](float* dst, uint16_t* dst_bf, size_t goff, long long len, xq_dqn::PendingSlab& p) {
        t.dst[k] = dst; t.dst_bf[k] = dst_bf; t.src[k] = G + goff; t.len[k] = len; t.state_off[k] = (long long)goff;
        if (p.nslabs > 0) { t.src[k] = p.src; t.nslabs[k] = p.nslabs; t.stride[k] = p.stride; }     // summed by the apply (or the norm) itself
        p = xq_dqn::PendingSlab();
        ++k;
    });
    t.nseg = k;
    params_written(d, ParamWrite::TD_SEGMENTS);
    ClipArgs C; memset(&C, 0, sizeof C);
    const bool clip = d->clip_max_norm > 0.0;
    if (clip) XQ_TRY(grad_norm(d, t, grad_scale, &C));
    // soft target update (xq_dqn_set_target_tau): inside the apply kernel while the nets agree outside the TD segments, else the plain
    // apply and one whole-buffer kernel behind it (the same element rule on the same values: the same bits); tau = 1 is the hard copy
    // (decided on tau32, the value the kernels use: a tau that rounds to 0 is off, one that rounds to 1 is the copy)
    const float tau32 = (float)d->target_tau;
    const bool soft = tau32 > 0.f && tau32 < 1.f;
    SoftArgs Z; memset(&Z, 0, sizeof Z);
    const bool fused_soft = soft && d->tgt_rest_synced;
    if (fused_soft) { soft_td_segments(d, &Z); Z.tau = tau32; }
    const SoftArgs* z = fused_soft ? &Z : nullptr;
    if (d->opt_kind == XQ_OPT_ADAM) XQ_TRY(adam_apply(d, t, lr, grad_scale, clip ? &C : nullptr, z));
    else XQ_TRY(sgd_apply(d, t, lr * grad_scale, clip ? &C : nullptr, z));
    if (soft && !fused_soft) return soft_target_whole(d, d->target_tau);
    if (tau32 == 1.f) return xq_dqn_update_target(d);
    return XQ_OK;
}

int xq_dqn_set_target_tau(xq_dqn* d, double tau) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (!(tau >= 0.0 && tau <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_target_tau: tau must lie in [0, 1] (0 = off, 1 = the hard copy)");
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_target_tau: a TD step is waiting for its apply_grads");
    d->target_tau = tau;
    return XQ_OK;
}

int xq_dqn_get_target_tau(const xq_dqn* d, double* tau) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (tau) *tau = d->target_tau;
    return XQ_OK;
}

int xq_dqn_soft_update_target(xq_dqn* d, double tau) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (!(tau >= 0.0 && tau <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_soft_update_target: tau must lie in [0, 1]");
    if ((float)tau == 0.f) return XQ_OK;
    if ((float)tau == 1.f) return xq_dqn_update_target(d);
    return soft_target_whole(d, tau);
}

// m = v = 0, t = 0 (queued on the handle's stream, behind any apply in flight)
static int adam_zero_state(xq_dqn* d) {
    d->opt_t = 0;
    if (!d->adam_m.p) return XQ_OK;
    XQ_HIP(hipMemsetAsync(d->adam_m, 0, d->n_grads_td * sizeof(float), d->stream));
    XQ_HIP(hipMemsetAsync(d->adam_v, 0, d->n_grads_td * sizeof(float), d->stream));
    return XQ_OK;
}

int xq_dqn_set_optimizer(xq_dqn* d, int kind, double beta1, double beta2, double eps) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (kind != XQ_OPT_SGD && kind != XQ_OPT_ADAM) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_optimizer: unknown optimizer kind %d", kind);
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_optimizer: beta1, beta2 must lie in [0, 1) and eps must not be negative");
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_optimizer: a TD step is waiting for its apply_grads");
    if (kind == XQ_OPT_ADAM && !d->adam_m.p) {
        if (d->n_grads_td == 0) layout_td_grads(d);
        XQ_TRY(d->adam_m.alloc(d->n_grads_td));
        XQ_TRY(d->adam_v.alloc(d->n_grads_td));
        XQ_TRY(adam_zero_state(d));
    }
    if (kind != d->opt_kind) XQ_TRY(adam_zero_state(d));
    d->opt_kind = kind;
    d->opt_b1 = beta1 != 0.0 ? beta1 : 0.9;
    d->opt_b2 = beta2 != 0.0 ? beta2 : 0.999;
    d->opt_eps = eps != 0.0 ? eps : 1e-8;
    return XQ_OK;
}

int xq_dqn_get_optimizer(const xq_dqn* d, int* kind, double* beta1, double* beta2, double* eps, uint64_t* steps) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (kind) *kind = d->opt_kind;
    if (beta1) *beta1 = d->opt_b1;
    if (beta2) *beta2 = d->opt_b2;
    if (eps) *eps = d->opt_eps;
    if (steps) *steps = d->opt_t;
    return XQ_OK;
}

int xq_dqn_reset_optimizer(xq_dqn* d) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    return adam_zero_state(d);
}

int xq_dqn_get_optimizer_state(xq_dqn* d, float* m_host, float* v_host, uint64_t* steps) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (d->opt_kind != XQ_OPT_ADAM) return fail(XQ_ERR_RUNTIME, "xq_dqn_get_optimizer_state: the optimizer is SGD, which keeps no state");
    XQ_HIP(hipStreamSynchronize(d->stream));
    if (m_host) XQ_HIP(hipMemcpy(m_host, d->adam_m, d->n_grads_td * sizeof(float), hipMemcpyDeviceToHost));
    if (v_host) XQ_HIP(hipMemcpy(v_host, d->adam_v, d->n_grads_td * sizeof(float), hipMemcpyDeviceToHost));
    if (steps) *steps = d->opt_t;
    return XQ_OK;
}

int xq_dqn_set_optimizer_state(xq_dqn* d, const float* m_host, const float* v_host, uint64_t steps) {
    if (!d || !m_host || !v_host) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_optimizer_state: null pointer");
    if (d->opt_kind != XQ_OPT_ADAM) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_optimizer_state: the optimizer is SGD, which keeps no state");
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_optimizer_state: a TD step is waiting for its apply_grads");
    XQ_HIP(hipStreamSynchronize(d->stream));
    XQ_HIP(hipMemcpy(d->adam_m, m_host, d->n_grads_td * sizeof(float), hipMemcpyHostToDevice));
    XQ_HIP(hipMemcpy(d->adam_v, v_host, d->n_grads_td * sizeof(float), hipMemcpyHostToDevice));
    d->opt_t = steps;
    return XQ_OK;
}

int xq_dqn_set_grad_clip(xq_dqn* d, double max_norm) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (!(max_norm >= 0.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_grad_clip: max_norm must be 0 (off), positive or +inf");
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_grad_clip: a TD step is waiting for its apply_grads");
    if (max_norm > 0.0 && d->clip_max_norm == 0.0) {            // switched on: norm, coefficient and both counters start at 0
        if (!d->clip_rec.p) {
            XQ_TRY(d->clip_partials.alloc(kNormMaxPartials));
            XQ_TRY(d->clip_rec.alloc(1));
        }
        XQ_HIP(hipMemsetAsync(d->clip_rec, 0, sizeof(ClipRecord), d->stream));
    }
    d->clip_max_norm = max_norm;
    return XQ_OK;
}

int xq_dqn_get_grad_clip(const xq_dqn* d, double* max_norm) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (max_norm) *max_norm = d->clip_max_norm;
    return XQ_OK;
}

int xq_dqn_grad_clip_stats(xq_dqn* d, double* last_norm, double* last_coef, uint64_t* applies, uint64_t* clipped) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (!(d->clip_max_norm > 0.0)) return fail(XQ_ERR_RUNTIME, "xq_dqn_grad_clip_stats: gradient clipping is off");
    ClipRecord r;
    XQ_HIP(hipStreamSynchronize(d->stream));
    XQ_HIP(hipMemcpy(&r, d->clip_rec, sizeof r, hipMemcpyDeviceToHost));
    if (last_norm) *last_norm = r.norm;
    if (last_coef) *last_coef = r.coef;
    if (applies) *applies = r.applies;
    if (clipped) *clipped = r.clipped;
    return XQ_OK;
}

int xq_dqn_set_td_loss(xq_dqn* d, int kind, double kappa) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (kind != XQ_LOSS_SQUARED && kind != XQ_LOSS_HUBER) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_td_loss: unknown loss %d", kind);
    // (the kernels clamp at (float)kappa: one that rounds to 0 there would clamp every error to 0)
    const float k32 = kappa > (double)FLT_MAX ? std::numeric_limits<float>::infinity() : (float)kappa;
    if (kind == XQ_LOSS_HUBER && !(kappa > 0.0 && k32 > 0.f))
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_td_loss: kappa must be positive or +inf");
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_td_loss: a TD step is waiting for its apply_grads");
    d->loss_kind = kind;
    if (kind == XQ_LOSS_HUBER) {
        d->loss_kappa = kappa;
        d->loss_kappa32 = k32;
    }
    return XQ_OK;
}

int xq_dqn_get_td_loss(const xq_dqn* d, int* kind, double* kappa) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (kind) *kind = d->loss_kind;
    if (kappa) *kappa = d->loss_kappa;
    return XQ_OK;
}

int xq_dqn_td_error_stats(xq_dqn* d, uint64_t* live, double* mean_abs, double* max_abs, double* mean_loss, uint64_t* linear) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (d->last_n <= 0) return fail(XQ_ERR_RUNTIME, "xq_dqn_td_error_stats: no TD step has run yet");
    if (!d->td_stats_rec.p) XQ_TRY(d->td_stats_rec.alloc(1));
    const float kappa = d->loss_kind == XQ_LOSS_HUBER ? d->loss_kappa32 : std::numeric_limits<float>::infinity();
    hipLaunchKernelGGL(td_error_stats_kernel, dim3(1), dim3(256), 0, d->stream, d->qsa.p, d->yv.p, d->act_mb.p, d->last_n, kappa, d->td_stats_rec.p);
    XQ_HIP(hipGetLastError());
    TdStatsRecord r;
    XQ_HIP(hipStreamSynchronize(d->stream));
    XQ_HIP(hipMemcpy(&r, d->td_stats_rec, sizeof r, hipMemcpyDeviceToHost));
    if (live) *live = r.live;
    if (mean_abs) *mean_abs = r.live ? r.sum_abs / (double)r.live : 0.0;
    if (max_abs) *max_abs = r.max_abs;
    if (mean_loss) *mean_loss = r.live ? r.sum_loss / (double)r.live : 0.0;
    if (linear) *linear = r.linear;
    return XQ_OK;
}

int xq_dqn_set_fused_apply(xq_dqn* d, int on) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_fused_apply: a TD step is waiting for its apply_grads");
    d->fused_apply = on != 0;
    return XQ_OK;
}

int xq_dqn_grad_buffer(xq_dqn* d, float** grads_dev, size_t* n_floats) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (grads_dev) *grads_dev = d->grads_td;
    if (n_floats) *n_floats = d->n_grads_td;
    return XQ_OK;
}

// ---- the staging pipeline of a TD step from a ring (DESIGN.md §4 "Staging pipeline") --------------------------------------------------
StageIo StagedBatch::io(const ReplayDev* ring) const {
    StageIo io; memset(&io, 0, sizeof io);
    if (ring) {
        io.boards = ring->boards; io.next_boards = ring->next_boards; io.action_to = ring->action_to; io.reward = ring->reward; io.done = ring->done;
        io.gather = 1u;
    } else {
        io.boards = ns_boards; io.next_boards = ns_next; io.action_to = ns_action; io.reward = ns_reward; io.done = ns_done;
    }
    io.s_boards = ns_boards; io.s_next = ns_next; io.s_action = ns_action; io.s_reward = ns_reward; io.s_done = ns_done; io.s_first = ns_first;
    return io;
}

// The flag stream of a random transform's next launch, {b, 0, *calls, stream word} of the ring's Philox; counts the launch
static StageDraw stage_draw(const xq_replay* r, double prob, uint64_t* calls) {
    const StageDraw dr = {eps_to_u32(prob), prob >= 1.0 ? 1u : 0u, (uint32_t)*calls, (uint32_t)r->seed, (uint32_t)(r->seed >> 32)};
    *calls += 1;
    return dr;
}

// Each stage below queues its kernel for the next TD step from ring `r`.  gather: the minibatch from the ring (through `src`) into the
// staging batch; otherwise the staging batch that the stages before it filled, in place.  row_next: in place, the column of the slots
// whose s' the rows hold

// n-step returns (xq_replay_set_n_step): assembles the n-step transitions; *disc_n: the step's discount, gamma^n
static int nstep_assemble(xq_dqn* d, xq_replay* r, SlotSrc src, int batch, float* disc_n) {
    StagedBatch& sb = d->staged;
    const int cap = r->dev.capacity, n = r->n_step;
    NStepArgs A; memset(&A, 0, sizeof A);
    A.boards = r->dev.boards; A.next_boards = r->dev.next_boards; A.action_to = r->dev.action_to; A.reward = r->dev.reward; A.done = r->dev.done;
    A.cap = cap; A.stride = r->n_stride; A.n = n;
    const RingSpan range = r->read_count >= 0 ? RingSpan{r->read_first, r->read_count} : ring_filled(ring_state(r));
    A.first = range.first; A.count = range.count;
    r->read_count = -1;                              // a narrowed range holds for one step
    if (!range.inside(cap)) return fail(XQ_ERR_INVALID_ARGUMENT, "n-step readable range (%d, %d) outside the ring", A.first, A.count);
    const float gf = d->zero_sum ? -(float)d->gamma : (float)d->gamma;      // zero-sum: disc_k = (-1)^k g^k, the chain's movers alternate
    float dk[kNStepMax + 1];                         // disc_k: float times float, one fp32 rounding per factor
    dk[0] = 1.f;
    for (int k = 1; k <= kNStepMax; ++k) dk[k] = dk[k - 1] * gf;
    for (int k = 0; k < kNStepMax; ++k) A.disc[k] = dk[k];
    *disc_n = dk[n];
    XQ_TRY(sb.reserve((size_t)batch));
    for (DevBuf<int32_t>* b : {&sb.ns_m, &sb.ns_last}) XQ_TRY(b->reserve((size_t)batch));
    A.s_boards = sb.ns_boards; A.s_next = sb.ns_next; A.s_action = sb.ns_action; A.s_reward = sb.ns_reward; A.s_done = sb.ns_done;
    A.s_m = sb.ns_m; A.s_first = sb.ns_first; A.s_last = sb.ns_last;
    // per row: n x 9 B of chain fields and two boards in, two boards and 21 B out
    ProfScope ps(d, "nstep_assemble", 0.0, (double)batch * (9.0 * n + 4.0 * 48 + 21), true);
    hipExtLaunchKernelGGL(nstep_assemble_kernel, dim3((batch + 63) / 64), dim3(64), 0, d->cur, ps.start(), ps.stop(), 0, A, src, batch);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// Mirror augmentation (xq_replay_set_mirror): whether row b is reflected is the ring's Philox stream at {b, 0, call, 3}
static int mirror_stage(xq_dqn* d, xq_replay* r, SlotSrc src, int batch, bool gather) {
    StagedBatch& sb = d->staged;
    if (gather) XQ_TRY(sb.reserve((size_t)batch));
    XQ_TRY(sb.ns_flag.reserve((size_t)batch));
    MirrorArgs A; memset(&A, 0, sizeof A);
    A.io = sb.io(gather ? &r->dev : nullptr);
    A.draw = stage_draw(r, r->mirror_prob, &r->mirror_calls);
    A.s_flag = sb.ns_flag;
    // per row, from the ring: two boards and 9 B in, two boards, 9 B, the slot and the flag out; in place: two boards and the action
    // in, two boards, the action and the flag out
    ProfScope ps(d, "mirror_stage", 0.0, (double)batch * (gather ? 215.0 : 201.0), true);
    hipExtLaunchKernelGGL(mirror_stage_kernel, dim3((batch + 63) / 64), dim3(64), 0, d->cur, ps.start(), ps.stop(), 0, A, src, batch);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// Colour-swap augmentation (xq_replay_set_colour_swap): whether row b is swapped is the ring's Philox stream at {b, 0, call, 4}.  Under
// the legal-move bootstrap the kernel also stages the side bytes, from the ring's column at row_next[b] (gather: at the sampled slot),
// flipped on the flagged rows
static int colour_swap_stage(xq_dqn* d, xq_replay* r, SlotSrc src, int batch, bool gather, const DevBuf<int32_t>& row_next) {
    StagedBatch& sb = d->staged;
    const bool sided = d->bootstrap == XQ_BOOTSTRAP_LEGAL;
    if (gather) XQ_TRY(sb.reserve((size_t)batch));
    XQ_TRY(sb.ns_cflag.reserve((size_t)batch));
    if (sided) XQ_TRY(sb.ns_side.reserve((size_t)batch));
    ColourSwapArgs A; memset(&A, 0, sizeof A);
    A.io = sb.io(gather ? &r->dev : nullptr);
    A.draw = stage_draw(r, r->colour_swap_prob, &r->colour_swap_calls);
    A.s_flag = sb.ns_cflag;
    if (sided) { A.ring_side = r->dev.next_player; A.row_slot = gather ? nullptr : row_next.p; A.s_side = sb.ns_side; }
    A.cap = r->dev.capacity;
    // per row: the mirror's bytes (from the ring 215, in place 201); under the legal bootstrap the ring's side byte in and the staged
    // one out, in place also the 4 B of the slot it is read at
    const double side_bytes = sided ? (gather ? 2.0 : 6.0) : 0.0;
    ProfScope ps(d, "colour_swap_stage", 0.0, (double)batch * ((gather ? 215.0 : 201.0) + side_bytes), true);
    hipExtLaunchKernelGGL(colour_swap_stage_kernel, dim3((batch + 63) / 64), dim3(64), 0, d->cur, ps.start(), ps.stop(), 0, A, src, batch);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// Mover view (xq_dqn_set_view): s flagged by the ring's mover column at the sampled slot (in place: ns_first[b]) and s' by its
// next_player column at the slot of s' (in place: row_next[b]).  Under the legal-move bootstrap the kernel stages the side bytes too —
// 0 on every row, the view of s' has Red to move
static int mover_view_stage(xq_dqn* d, xq_replay* r, SlotSrc src, int batch, bool gather, const DevBuf<int32_t>& row_next) {
    StagedBatch& sb = d->staged;
    const bool sided = d->bootstrap == XQ_BOOTSTRAP_LEGAL;
    if (gather) XQ_TRY(sb.reserve((size_t)batch));
    XQ_TRY(sb.ns_vflag.reserve((size_t)batch));
    XQ_TRY(sb.ns_vflag_next.reserve((size_t)batch));
    if (sided) XQ_TRY(sb.ns_side.reserve((size_t)batch));
    MoverViewArgs A; memset(&A, 0, sizeof A);
    A.io = sb.io(gather ? &r->dev : nullptr);
    if (!gather) { A.row_first = sb.ns_first; A.row_last = row_next.p; }
    A.s_flag = sb.ns_vflag; A.s_flag_next = sb.ns_vflag_next;
    A.mover = r->dev.mover; A.next_player = r->dev.next_player;
    if (sided) A.s_side = sb.ns_side;
    A.cap = r->dev.capacity;
    // per row: the mirror's bytes (from the ring 215, in place 201) with a second flag out, the two side bytes in, in place the 8 B
    // of the two slots they are read at; under the legal bootstrap the staged side byte out
    ProfScope ps(d, "mover_view_stage", 0.0, (double)batch * ((gather ? 218.0 : 212.0) + (sided ? 1.0 : 0.0)), true);
    hipExtLaunchKernelGGL(mover_view_stage_kernel, dim3((batch + 63) / 64), dim3(64), 0, d->cur, ps.start(), ps.stop(), 0, A, src, batch);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

// The TD step on the staging batch: identity slot source, the given discount (nullptr: the handle's gamma).  A prioritized draw keeps its
// importance weights; the step gets no priority table, and per_writeback_kernel behind it writes the live rows' priorities to the sampled
// slots recorded in ns_first.  Under the legal-move bootstrap the staged rows' side bytes come from the ring's column at row_next[b]
// (legal_side_stage_kernel) unless a transform has staged them already (side_staged)
static int td_grads_staged(xq_dqn* d, xq_replay* r, const DevBuf<int32_t>& row_next, int batch, int td_net, int mode, const PerOpts* per,
                           const float* discount, bool side_staged) {
    StagedBatch& sb = d->staged;
    PerOpts step_per;
    if (per) { step_per = *per; step_per.prio = nullptr; step_per.pmax_live = nullptr; }
    const bool legal = d->bootstrap == XQ_BOOTSTRAP_LEGAL;
    if (legal && !side_staged) {
        XQ_TRY(sb.ns_side.reserve((size_t)batch));
        ProfScope ps(d, "legal_side_stage", 0.0, (double)batch * 6.0, true);
        hipExtLaunchKernelGGL(legal_side_stage_kernel, dim3((batch + 255) / 256), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0,
                              r->dev.next_player, row_next.p, sb.ns_side.p, batch, r->dev.capacity);
        XQ_HIP(hipGetLastError());
    }
    XQ_TRY(td_grads_impl(d, sb.ns_boards, sb.ns_next, sb.ns_action, sb.ns_reward, sb.ns_done, explicit_slots(nullptr), batch, td_net, mode,
                         per ? &step_per : nullptr, discount, legal ? sb.ns_side.p : nullptr));
    if (per) {
        ProfScope ps(d, "per_writeback", 0.0, (double)batch * 20.0, true);
        hipExtLaunchKernelGGL(per_writeback_kernel, dim3((batch + 255) / 256), dim3(256), 0, d->cur, ps.start(), ps.stop(), 0, batch,
                              d->qsa.p, d->yv.p, d->act_mb.p, sb.ns_first.p, per->prio, per->pmax_live, per->eps, per->alpha);
        XQ_HIP(hipGetLastError());
    }
    return XQ_OK;
}

// A TD step from ring `r` with at least one staging stage on.  The stages run in one fixed order — assemble, mirror, colour swap, view
// (the last two never together: xq_dqn_td_grads_replay refuses the pair; mirror and colour swap commute, one acts on columns, the
// other on rows and codes) — the first of them gathers from the ring and every later one works in place.  The slots of s' are ns_last
// behind the assembly and the sampled slots otherwise: the colour swap and the view read the ring's side there, and under the legal
// bootstrap so does legal_side_stage_kernel when neither of them ran.  The step then runs on the batch with the n-step discount or the
// handle's; a prioritized draw's priorities go back to the sampled slots behind it
static int td_grads_ring_staged(xq_dqn* d, xq_replay* r, SlotSrc src, int batch, int td_net, int mode, const PerOpts* per) {
    StagedBatch& sb = d->staged;
    const bool assembled = r->n_step > 1;
    const DevBuf<int32_t>& row_next = assembled ? sb.ns_last : sb.ns_first;
    const bool legal = d->bootstrap == XQ_BOOTSTRAP_LEGAL;
    unsigned stages = 0;                             // == 0: the batch is not filled yet, the next stage gathers
    bool sided = false;
    float disc_n = 0.f;
    if (assembled) { XQ_TRY(nstep_assemble(d, r, src, batch, &disc_n)); stages |= StagedBatch::kAssemble; }
    if (r->mirror_prob > 0.0) { XQ_TRY(mirror_stage(d, r, src, batch, stages == 0)); stages |= StagedBatch::kMirror; }
    if (r->colour_swap_prob > 0.0) {
        XQ_TRY(colour_swap_stage(d, r, src, batch, stages == 0, row_next));
        stages |= StagedBatch::kColourSwap; sided = legal;
    }
    if (d->view == XQ_VIEW_MOVER) {
        XQ_TRY(mover_view_stage(d, r, src, batch, stages == 0, row_next));
        stages |= StagedBatch::kView; sided = legal;
    }
    XQ_TRY(td_grads_staged(d, r, row_next, batch, td_net, mode, per, assembled ? &disc_n : nullptr, sided));
    sb.last = {batch, stages, sided};
    return XQ_OK;
}

// ---- read-back of the last step's staging batch (xq_dqn_last_*) ------------------------------------------------------------------------
// The checks they share: the handle, that `stage` ran in the last TD step (`what`: "a mirror-mode", ...), n within its rows
static int last_staged_rows(const xq_dqn* d, unsigned stage, int n, const char* fn, const char* what) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    const StagedBatch::Last& last = d->staged.last;
    if (!(last.stages & stage)) return fail(XQ_ERR_RUNTIME, "%s: the last TD step was not %s one", fn, what);
    if (n < 0 || n > last.rows) return fail(XQ_ERR_INVALID_ARGUMENT, "%s: n exceeds the last TD step's %d rows", fn, last.rows);
    return XQ_OK;
}

static int staged_column(void* out, const void* col, int n, size_t elem = 1) {        // rows 0..n-1 of a column, if asked for
    if (out && n) XQ_HIP(hipMemcpy(out, col, (size_t)n * elem, hipMemcpyDeviceToHost));
    return XQ_OK;
}

// Waits for the step, then copies what every transform's read-back returns: both boards (unpacked), the action and the sampled slot
static int last_staged_batch(xq_dqn* d, int n, uint8_t* boards90, uint8_t* next_boards90, int32_t* action_to, int32_t* slot) {
    const StagedBatch& sb = d->staged;
    XQ_HIP(hipStreamSynchronize(d->stream));
    if (!n) return XQ_OK;
    std::vector<uint32_t> w((size_t)n * kBoardWords);
    const struct { uint8_t* out; const uint32_t* dev; } boards[2] = {{boards90, sb.ns_boards}, {next_boards90, sb.ns_next}};
    for (const auto& bd : boards) {
        if (!bd.out) continue;
        XQ_HIP(hipMemcpy(w.data(), bd.dev, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) unpack_board(&w[(size_t)i * kBoardWords], bd.out + (size_t)i * 90);
    }
    XQ_TRY(staged_column(action_to, sb.ns_action, n, sizeof(int32_t)));
    return staged_column(slot, sb.ns_first, n, sizeof(int32_t));
}

int xq_dqn_last_n_step(xq_dqn* d, int n, float* reward, uint8_t* done, int32_t* steps, int32_t* first_slot, int32_t* last_slot,
                       int32_t* action) {
    XQ_TRY(last_staged_rows(d, StagedBatch::kAssemble, n, "xq_dqn_last_n_step", "an n-step"));
    XQ_TRY(last_staged_batch(d, n, nullptr, nullptr, action, first_slot));
    const StagedBatch& sb = d->staged;
    XQ_TRY(staged_column(reward, sb.ns_reward, n, sizeof(float)));
    XQ_TRY(staged_column(done, sb.ns_done, n));
    XQ_TRY(staged_column(steps, sb.ns_m, n, sizeof(int32_t)));
    return staged_column(last_slot, sb.ns_last, n, sizeof(int32_t));
}

int xq_dqn_last_mirror(xq_dqn* d, int n, uint8_t* flags, uint8_t* boards90, uint8_t* next_boards90, int32_t* action_to, int32_t* slot) {
    XQ_TRY(last_staged_rows(d, StagedBatch::kMirror, n, "xq_dqn_last_mirror", "a mirror-mode"));
    XQ_TRY(last_staged_batch(d, n, boards90, next_boards90, action_to, slot));
    return staged_column(flags, d->staged.ns_flag, n);
}

int xq_dqn_last_colour_swap(xq_dqn* d, int n, uint8_t* flags, uint8_t* boards90, uint8_t* next_boards90, int32_t* action_to,
                            uint8_t* next_player, int32_t* slot) {
    XQ_TRY(last_staged_rows(d, StagedBatch::kColourSwap, n, "xq_dqn_last_colour_swap", "a colour-swap-mode"));
    if (next_player && !d->staged.last.sided)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_last_colour_swap: next_player asked, but the last TD step was not under the legal-move bootstrap");
    XQ_TRY(last_staged_batch(d, n, boards90, next_boards90, action_to, slot));
    XQ_TRY(staged_column(flags, d->staged.ns_cflag, n));
    return staged_column(next_player, d->staged.ns_side, n);
}

int xq_dqn_last_view(xq_dqn* d, int n, uint8_t* flag_s, uint8_t* flag_next, uint8_t* boards90, uint8_t* next_boards90, int32_t* action_to,
                     int32_t* slot) {
    XQ_TRY(last_staged_rows(d, StagedBatch::kView, n, "xq_dqn_last_view", "a view-mode"));
    XQ_TRY(last_staged_batch(d, n, boards90, next_boards90, action_to, slot));
    XQ_TRY(staged_column(flag_s, d->staged.ns_vflag, n));
    return staged_column(flag_next, d->staged.ns_vflag_next, n);
}

int xq_dqn_td_grads_replay(xq_dqn* d, xq_replay* r, int batch, int td_net, int mode) {
    if (!d || !r) return fail(XQ_ERR_INVALID_ARGUMENT, "null handle");
    SlotSrc src = explicit_slots(nullptr);
    if (batch > 0) {
        if (r->last_batch != batch) return fail(XQ_ERR_INVALID_ARGUMENT, "call xq_replay_sample(batch) first");
        if (r->implicit) {                  // the trainer's virtual sample: slots recomputed inside the consumer kernels
            src.implicit = 1; src.call = r->implicit_call; src.size = (uint32_t)r->implicit_size;
            src.start = (uint32_t)r->implicit_start; src.cap = (uint32_t)r->dev.capacity;
            src.seed_lo = (uint32_t)r->seed; src.seed_hi = (uint32_t)(r->seed >> 32);
        } else {
            if (!r->slots_dev) return fail(XQ_ERR_INVALID_ARGUMENT, "call xq_replay_sample(batch) first");
            src.slots = r->slots_dev;
        }
    } else {
        batch = r->size;       // identity over the filled part of the ring (on-policy use)
    }
    if (batch <= 0) return fail(XQ_ERR_RUNTIME, "replay is empty");
    if (d->bootstrap == XQ_BOOTSTRAP_LEGAL && !r->dev.next_player)
        return fail(XQ_ERR_INVALID_ARGUMENT, "the legal-move bootstrap needs the side to move in s': this ring does not track it (xq_replay_track_next_player)");
    const bool viewed = d->view == XQ_VIEW_MOVER;
    if (viewed && (!r->dev.mover || !r->dev.next_player))
        return fail(XQ_ERR_INVALID_ARGUMENT, "the mover view needs who moved and who moves next: this ring does not track both "
                                             "(xq_replay_track_mover, xq_replay_track_next_player)");
    if (viewed && r->colour_swap_prob > 0.0)
        return fail(XQ_ERR_INVALID_ARGUMENT, "the mover view (xq_dqn_set_view) and colour-swap augmentation (xq_replay_set_colour_swap) are both "
                                             "on: the view of a swapped transition is the view of the transition, switch one of them off");
    PerOpts per; memset(&per, 0, sizeof per);
    const bool prioritized = r->per.enabled && r->per.last_prioritized && !r->implicit && src.slots != nullptr;
    if (prioritized) {        // importance weights in, TD-error priorities out (xq_replay_sample_prioritized drew the slots)
        per.is_w = r->per.is_w; per.is_wmax = reinterpret_cast<const float*>(r->per.scalars + 2);
        per.prio = r->dev.prio; per.pmax_live = r->per.scalars + 0;
        per.eps = r->per.eps; per.alpha = r->per.alpha;
    }
    // ring, slot list and priorities may have been written on other streams (env steps, the draw, a rebuild): this step starts behind
    // them, and whatever touches them next — the next draw overwrites the list, the next env step the slots — behind this step
    XQ_TRY(replay_consumer_begin(r, d->stream, src.slots != nullptr, prioritized));
    if (r->n_step > 1 || r->mirror_prob > 0.0 || r->colour_swap_prob > 0.0 || viewed)
        return td_grads_ring_staged(d, r, src, batch, td_net, mode, prioritized ? &per : nullptr);
    return td_grads_impl(d, r->dev.boards, r->dev.next_boards, r->dev.action_to, r->dev.reward, r->dev.done, src, batch, td_net,
                         mode, prioritized ? &per : nullptr, nullptr, r->dev.next_player);
}

static int td_update_host_impl(xq_dqn* d, int n, const uint8_t* boards90, const uint8_t* next_boards90, const int32_t* action_to,
                               const float* reward, const uint8_t* done, const uint8_t* next_player, int td_net, int mode, double lr,
                               double grad_scale, float* q_sa_out, float* y_out) {
    if (!d || n <= 0 || !boards90 || !next_boards90 || !action_to || !reward || !done)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_td_update_host: bad argument");
    if (next_player) {
        for (int i = 0; i < n; ++i) {
            if (next_player[i] > 1) return fail(XQ_ERR_INVALID_ARGUMENT, "next_player[%d] = %d: 0 (Red) or 1 (Black)", i, (int)next_player[i]);
            // (move generation ranks a side's pieces into a 16-entry table)
            if (const char* why = board_fault(next_boards90 + (size_t)i * 90)) return fail(XQ_ERR_INVALID_ARGUMENT, "next board %d: %s", i, why);
        }
        XQ_TRY(d->hside.reserve((size_t)n));
    }
    for (size_t i = 0; i < (size_t)n * 90; ++i)       // code 15 would index one-hot plane 14 of 14 in the layer-0 kernels
        if (boards90[i] > 14 || next_boards90[i] > 14) return fail(XQ_ERR_INVALID_ARGUMENT, "piece code > 14");
    XQ_TRY(d->hb.reserve((size_t)n * 2 * kBoardWords));
    XQ_TRY(d->ha.reserve((size_t)n));
    XQ_TRY(d->hr.reserve((size_t)n));
    XQ_TRY(d->hd.reserve((size_t)n));
    std::vector<uint32_t> w((size_t)n * 2 * kBoardWords);
    for (int i = 0; i < n; ++i) {
        pack_board(boards90 + (size_t)i * 90, &w[(size_t)i * kBoardWords]);
        pack_board(next_boards90 + (size_t)i * 90, &w[((size_t)n + i) * kBoardWords]);
    }
    XQ_HIP(hipStreamSynchronize(d->stream));
    XQ_HIP(hipMemcpy(d->hb, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    XQ_HIP(hipMemcpy(d->ha, action_to, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    XQ_HIP(hipMemcpy(d->hr, reward, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    XQ_HIP(hipMemcpy(d->hd, done, (size_t)n, hipMemcpyHostToDevice));
    if (next_player) XQ_HIP(hipMemcpy(d->hside, next_player, (size_t)n, hipMemcpyHostToDevice));
    XQ_TRY(td_grads_impl(d, d->hb, d->hb + (size_t)n * kBoardWords, d->ha, d->hr, d->hd, explicit_slots(nullptr), n, td_net, mode, nullptr, nullptr,
                         next_player ? d->hside.p : nullptr));
    XQ_TRY(xq_dqn_apply_grads(d, lr, grad_scale));
    XQ_HIP(hipStreamSynchronize(d->stream));
    if (q_sa_out) XQ_HIP(hipMemcpy(q_sa_out, d->qsa, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (y_out) XQ_HIP(hipMemcpy(y_out, d->yv, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return XQ_OK;
}
int xq_dqn_td_update_host(xq_dqn* d, int n, const uint8_t* boards90, const uint8_t* next_boards90, const int32_t* action_to,
                          const float* reward, const uint8_t* done, int td_net, int mode, double lr, double grad_scale,
                          float* q_sa_out, float* y_out) {
    return td_update_host_impl(d, n, boards90, next_boards90, action_to, reward, done, nullptr, td_net, mode, lr, grad_scale, q_sa_out, y_out);
}
int xq_dqn_td_update_host_sided(xq_dqn* d, int n, const uint8_t* boards90, const uint8_t* next_boards90, const int32_t* action_to,
                                const float* reward, const uint8_t* done, const uint8_t* next_player, int td_net, int mode, double lr,
                                double grad_scale, float* q_sa_out, float* y_out) {
    if (!next_player) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_td_update_host_sided: null next_player");
    return td_update_host_impl(d, n, boards90, next_boards90, action_to, reward, done, next_player, td_net, mode, lr, grad_scale, q_sa_out, y_out);
}

int xq_dqn_set_td_bootstrap(xq_dqn* d, int kind) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (kind != XQ_BOOTSTRAP_ALL && kind != XQ_BOOTSTRAP_LEGAL) return fail(XQ_ERR_INVALID_ARGUMENT, "unknown TD bootstrap %d", kind);
    if (kind == XQ_BOOTSTRAP_LEGAL && d->nout() < 96) return fail(XQ_ERR_INVALID_ARGUMENT, "the legal-move bootstrap needs >= 96 outputs");
    d->bootstrap = kind;
    return XQ_OK;
}
int xq_dqn_get_td_bootstrap(const xq_dqn* d, int* kind) {
    if (!d || !kind) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    *kind = d->bootstrap;
    return XQ_OK;
}
int xq_dqn_set_zero_sum(xq_dqn* d, int on) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (on != 0 && on != 1) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_zero_sum: on must be 0 or 1, got %d", on);
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_zero_sum: a TD step is waiting for its apply_grads");
    d->zero_sum = on;
    return XQ_OK;
}
int xq_dqn_get_zero_sum(const xq_dqn* d, int* on) {
    if (!d || !on) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    *on = d->zero_sum;
    return XQ_OK;
}
int xq_dqn_set_view(xq_dqn* d, int view) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (view != XQ_VIEW_ABSOLUTE && view != XQ_VIEW_MOVER) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_set_view: unknown view %d", view);
    if (td_step_pending(d)) return fail(XQ_ERR_RUNTIME, "xq_dqn_set_view: a TD step is waiting for its apply_grads");
    d->view = view;
    return XQ_OK;
}
int xq_dqn_get_view(const xq_dqn* d, int* view) {
    if (!d || !view) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    *view = d->view;
    return XQ_OK;
}
int xq_view_boards_dev(const void* boards_dev, const void* side_dev, int n, void* out_dev, void* hip_stream) {
    if (!boards_dev || !side_dev || !out_dev || n < 0) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_view_boards_dev: bad argument");
    if (boards_dev == out_dev) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_view_boards_dev: out_dev must not be boards_dev");
    return view_boards_launch(static_cast<const uint32_t*>(boards_dev), static_cast<const uint8_t*>(side_dev), nullptr, n,
                              static_cast<uint32_t*>(out_dev), static_cast<hipStream_t>(hip_stream));
}
int xq_dqn_last_legal(xq_dqn* d, int n, int32_t* n_moves, int32_t* a_star, float* zmax, float* z96) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    if (d->legal_rows <= 0) return fail(XQ_ERR_RUNTIME, "xq_dqn_last_legal: the last TD step was not a legal-bootstrap one");
    if (n < 0 || n > d->legal_rows) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_last_legal: n exceeds the last TD step's %d rows", d->legal_rows);
    XQ_HIP(hipStreamSynchronize(d->stream));
    if (!n) return XQ_OK;
    if (n_moves) XQ_HIP(hipMemcpy(n_moves, d->legal_nmoves, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (a_star) XQ_HIP(hipMemcpy(a_star, d->zidx, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (zmax) XQ_HIP(hipMemcpy(zmax, d->zmax, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (z96) XQ_HIP(hipMemcpy(z96, d->z96, (size_t)n * 96 * sizeof(float), hipMemcpyDeviceToHost));
    return XQ_OK;
}

int xq_dqn_last_loss(xq_dqn* d, double* loss) {
    if (!d || !loss) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    std::vector<float> v((size_t)std::max(d->last_n, 0));
    XQ_HIP(hipStreamSynchronize(d->stream));
    if (!v.empty()) XQ_HIP(hipMemcpy(v.data(), d->lossv, v.size() * sizeof(float), hipMemcpyDeviceToHost));
    double s = 0;
    for (float x : v) s += x;
    *loss = s;
    return XQ_OK;
}

int xq_dqn_last_td_values(xq_dqn* d, int n, float* q_sa_host, float* y_host) {
    if (!d || n < 0 || n > d->last_n) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_dqn_last_td_values: n exceeds the last TD step's %d samples", d ? d->last_n : 0);
    XQ_HIP(hipStreamSynchronize(d->stream));
    if (q_sa_host && n) XQ_HIP(hipMemcpy(q_sa_host, d->qsa, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (y_host && n) XQ_HIP(hipMemcpy(y_host, d->yv, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return XQ_OK;
}

int xq_dqn_kernel_stats(xq_dqn* d, int enable, xq_kernel_stat* stats, int max_stats, int* n_stats) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    XQ_HIP(hipStreamSynchronize(d->stream));
    d->prof.collect();
    int n = 0;
    if (stats && n_stats) {
        for (size_t i = 0; i < d->prof.cats.size() && n < max_stats; ++i, ++n) {
            const Profiler::Cat& c = d->prof.cats[i];
            memset(&stats[n], 0, sizeof stats[n]);
            strncpy(stats[n].name, c.name, sizeof stats[n].name - 1);
            stats[n].ms = c.ms; stats[n].launches = c.launches; stats[n].flops = c.flops; stats[n].bytes = c.bytes; stats[n].exact_launches = c.exact;
        }
    }
    if (n_stats) *n_stats = n;
    if (enable >= 0) {   // 0 off, 1 on, 2 on + clear, 3 on + clear, only the kernels bench.py prices (roofline leg), 4 = 3 sampled 1-in-4
        if ((enable != 0) != d->prof.enabled || enable >= 2) d->prof.reset();
        d->prof.enabled = enable != 0;
        d->prof.roofline_only = enable == 3 || enable == 4;
        d->prof.sample_period = enable == 4 ? 4 : 1;
        for (auto& o : d->prof.only) o.phase = 0;
    }
    return XQ_OK;
}

int xq_dqn_kernel_filter(xq_dqn* d, const char* names_csv) {
    if (!d) return fail(XQ_ERR_INVALID_ARGUMENT, "null dqn");
    d->prof.set_only(names_csv && *names_csv ? names_csv : "gemm_qmax_rowmax,gemm_qmax_screen,env_selfplay_step");
    return XQ_OK;
}

int xq_dqn_kernel_timeline(xq_dqn* d, xq_kernel_span* spans, int max_spans, int* n_spans) {
    if (!d || !n_spans) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    int n = 0;
    for (size_t i = 0; i < d->prof.spans.size() && spans && n < max_spans; ++i, ++n) {
        const Profiler::Span& sp = d->prof.spans[i];
        memset(&spans[n], 0, sizeof spans[n]);
        memcpy(spans[n].name, sp.name, sizeof spans[n].name);
        spans[n].start_ms = sp.start_ms; spans[n].end_ms = sp.end_ms;
    }
    *n_spans = n;
    return XQ_OK;
}

// DQN::saveModel / loadModel, dqn.cpp:76-154
static void put_be(FILE* f, uint64_t v, int bytes) { for (int i = bytes - 1; i >= 0; --i) fputc((int)((v >> (8 * i)) & 0xFF), f); }
static bool get_be(FILE* f, uint64_t* v, int bytes) {
    uint64_t x = 0;
    for (int i = 0; i < bytes; ++i) { int c = fgetc(f); if (c == EOF) return false; x = (x << 8) | (uint64_t)(c & 0xFF); }
    *v = x;
    return true;
}

int xq_dqn_save_model(xq_dqn* d, const char* path) {
    if (!d || !path) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    std::vector<double> w(d->nw), b(d->nb);
    XQ_TRY(xq_dqn_get_params(d, XQ_NET_ONLINE, w.data(), b.data()));
    FILE* f = fopen(path, "wb");
    if (!f) return fail(XQ_ERR_IO, "Unable to open file for saving model.");
    bool ok = fwrite(w.data(), sizeof(double), w.size(), f) == w.size();       // raw (little-endian host) fp64
    ok = ok && fwrite(b.data(), sizeof(double), b.size(), f) == b.size();
    put_be(f, (uint64_t)d->ns, 8);                                             // QDataStream: big-endian quint64
    for (int i = 0; i < d->ns; ++i) put_be(f, (uint64_t)(uint32_t)d->L[i], 4); // big-endian qint32
    ok = ok && !ferror(f);
    fclose(f);
    return ok ? XQ_OK : fail(XQ_ERR_IO, "Error writing weights to model file.");
}

int xq_dqn_load_model(xq_dqn* d, const char* path) {
    if (!d || !path) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(XQ_ERR_IO, "Unable to open file for loading model.");
    std::vector<double> w(d->nw), b(d->nb);
    bool ok = fread(w.data(), sizeof(double), w.size(), f) == w.size();
    ok = ok && fread(b.data(), sizeof(double), b.size(), f) == b.size();
    if (!ok) { fclose(f); return fail(XQ_ERR_IO, "Error reading weights from model file."); }
    uint64_t cnt = 0;
    ok = get_be(f, &cnt, 8);
    std::vector<int> sizes;
    for (uint64_t i = 0; ok && i < cnt && i < 64; ++i) { uint64_t v; ok = get_be(f, &v, 4); sizes.push_back((int)(uint32_t)v); }
    fclose(f);
    bool same = ok && cnt == (uint64_t)d->ns;
    for (int i = 0; same && i < d->ns; ++i) same = sizes[i] == d->L[i];
    if (!same) return fail(XQ_ERR_IO, "Layer sizes in the model file do not match the current network architecture.");
    return xq_dqn_set_params(d, XQ_NET_ONLINE, w.data(), b.data());           // qNetwork only, like upstream (:153)
}

}  // extern "C"
