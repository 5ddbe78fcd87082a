// xq_internal.h — handle layouts shared by the translation units of libxqhip (not part of the ABI).
#pragma once

#include "xq_common.h"
#include "xq_ring_window.h"

#include <algorithm>
#include <climits>
#include <utility>
#include <vector>

namespace xq {

// ---- ordering of device data shared between handles that run on different HIP streams ---------------------------------------------
// Classes of ordering the library provides (include/xq_capi.h, "Stream ordering"); xq_debug_set_stream_ordering switches them off one
// by one so that a test can show each of them is needed.
enum : unsigned { ORD_RING_CONTENTS = 1u, ORD_RING_PRIORITIES = 2u, ORD_RING_DRAW = 4u, ORD_TRAINER_PARAMS = 8u, ORD_ALL = 15u };
inline unsigned& order_mask() { static unsigned m = ORD_ALL; return m; }

// Flags of an event that only ever orders one device stream behind another (hipStreamWaitEvent; never hipEventSynchronize / Query):
// no timing and no system-scope fence when it completes — the consumer is a kernel on the same device, which acquires at device scope
// like any kernel behind another.  Measured (tools/sync_probe.hip): a record costs the recording stream 6.9 instead of 9.4 us between
// 6-us kernels; same-box A/B of the step 0.1739 -> 0.1715 ms.  XQ_EVENT_SYSFENCE=1 restores the fence (A/B knob).
inline unsigned stream_event_flags() {
    static const unsigned f = [] { const char* e = getenv("XQ_EVENT_SYSFENCE"); return (unsigned)hipEventDisableTiming | ((e && e[0] == '1') ? 0u : (unsigned)hipEventDisableSystemFence); }();
    return f;
}

// ---- the one owner of a HIP event, and of a handle's stream ------------------------------------------------------------------------
// Event: one hipEvent_t, destroyed by the destructor — a handle's events go with `delete handle`, a scoped one with its scope.  create()
// leaves an event that exists alone, which is the form the lazily created ones take (first use creates, later uses cost a test).  It
// converts to hipEvent_t wherever the handle is read.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(ev, o.ev); return *this; }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    operator hipEvent_t() const { return ev; }
    int create(unsigned flags) {       // stream_event_flags() for ordering events, hipEventDefault for the ones that time
        if (!ev) XQ_HIP(hipEventCreateWithFlags(&ev, flags));
        return XQ_OK;
    }
};

void retire_stream(hipStream_t s);     // xq_order.hip: strikes s from every SharedResource (below)

// Stream: the stream a handle runs on — its own, or one the caller lent (the void* hip_stream of every xq_*_create).  close() is the
// one teardown: synchronise, strike the stream from every SharedResource (nothing queued on it is left to wait for, and the caller
// may destroy a lent stream right after the handle), destroy it if it is the handle's own.  Closing twice, or closing a stream that
// was never opened (a handle whose init failed early), does nothing.  What stays with the xq_*_destroy functions is the ORDER: a side
// or collect stream before the main one, a stream lent to sub-handles after those sub-handles, every stream before `delete handle`
// frees the buffers its work may touch.  The destructor closes too, as a backstop.
struct Stream {
    static constexpr int kNoPriority = INT_MIN;
    hipStream_t s = nullptr;
    bool owned = false;
    Stream() = default;
    ~Stream() { close(); }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    operator hipStream_t() const { return s; }
    int open(void* lent) {             // the caller's stream, or a new one when there is none
        if (lent) { s = (hipStream_t)lent; return XQ_OK; }
        XQ_HIP(hipStreamCreate(&s));
        owned = true;
        return XQ_OK;
    }
    int open_owned(unsigned flags, int priority = kNoPriority) {
        if (priority == kNoPriority) XQ_HIP(hipStreamCreateWithFlags(&s, flags));
        else XQ_HIP(hipStreamCreateWithPriority(&s, flags, priority));
        owned = true;
        return XQ_OK;
    }
    void close() {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        retire_stream(s);
        if (owned) (void)hipStreamDestroy(s);
        s = nullptr; owned = false;
    }
};

// LazyMark: "everything `producer` has queued so far", for another stream to wait behind.  The record is made only when somebody is
// about to wait (it costs the recording stream ~6 us, and streams run in order, so a record made later still lies behind the work it
// stands for): touched() says the producer has queued work since the last record, wait() records if so and orders the consumer behind
// the event.  record() is the eager form, for the one place whose consumers must not see anything queued later.
struct LazyMark {
    Event ev;
    hipStream_t producer = nullptr;
    bool stale = false;                // the producer has queued work since the last record
    int open(hipStream_t producer_stream) { producer = producer_stream; return ev.create(stream_event_flags()); }
    void touched() { stale = true; }
    int record() {
        XQ_HIP(hipEventRecord(ev, producer));
        stale = false;
        return XQ_OK;
    }
    int wait(hipStream_t consumer) {
        if (stale) XQ_TRY(record());
        XQ_HIP(hipStreamWaitEvent(consumer, ev, 0));
        return XQ_OK;
    }
};

// One device resource and the streams that touched it last.  read(s) orders s behind the last write; write(s) orders s behind the
// last write and behind every read since.  The event is recorded LAZILY — on the producer's stream at the moment a consumer on another
// stream shows up (streams run in order, so a record made later still lies behind the producer's work) — because a record costs the
// recording stream ~6 us and most producers are never waited for.  A stream that goes away is struck from every
// resource first: Stream::close() (above) does it for every stream a handle holds — its own or the caller's — and xq_stream_destroy
// for the caller's own; a caller that destroys a lent stream while a handle still uses it gets its entries dropped at the next access
// (order_behind: a record on a dead stream fails, a dead stream has nothing left to wait for).
struct SharedResource {
    unsigned cls;
    bool has_writer = false;
    hipStream_t writer = nullptr;
    hipStream_t readers[4] = {nullptr, nullptr, nullptr, nullptr};
    int n_readers = 0;
    Event ev;                          // created by the first order_behind that has to wait
    explicit SharedResource(unsigned c);
    ~SharedResource();
    SharedResource(const SharedResource&) = delete;
    SharedResource& operator=(const SharedResource&) = delete;
    int order_behind(hipStream_t waiter, hipStream_t producer);
    int read(hipStream_t s);
    int write(hipStream_t s);
    void forget(hipStream_t s);        // s was synchronised and goes away (caller holds the registry's mutex: retire_stream, order_behind)
    void host_synchronised();          // the whole device was synchronised: nothing left to wait for
};

// ---- the one owner of device memory ----------------------------------------------------------------------------------------------
// DevBuf<T>: n elements of T in device memory (PinnedBuf<T>: in pinned host memory), freed by the destructor — a handle's buffers go
// with `delete handle`, a local scratch buffer with its scope, whichever way the function returns.  It converts to T* wherever the
// pointer is read (launch arguments, views such as ReplayDev, arithmetic); `p` names it where no conversion applies.
// reserve() is the one growth rule of the library: a buffer that is large enough costs no runtime call; one that is not is replaced
// behind a device-wide synchronise (whatever stream its last reader ran on — the select chain of a handle may be in flight on another
// stream than the handle's — has finished), the old contents are dropped, the new ones are undefined.  Callers that need zeros queue
// their own memset when `*grew` says so.  A failed alloc() / reserve() leaves the buffer empty, so a later call starts over.
struct DeviceMem {
    static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t put(void* p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t put(void* p) { return hipHostFree(p); }
};
template <class T, class Mem = DeviceMem>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;                      // elements
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    operator T*() const { return p; }
    void release() {
        if (p) (void)Mem::put(p);
        p = nullptr; n = 0;
    }
    int alloc(size_t count) {          // exactly `count` elements in place of whatever it holds
        release();
        void* q = nullptr;
        const hipError_t e = Mem::get(&q, count * sizeof(T));
        if (e != hipSuccess) return fail(XQ_ERR_RUNTIME, "HIP error: %s allocating %zu bytes", hipGetErrorString(e), count * sizeof(T));
        p = static_cast<T*>(q); n = count;
        return XQ_OK;
    }
    int reserve(size_t count, bool* grew = nullptr) {
        if (count <= n) return XQ_OK;
        XQ_HIP(hipDeviceSynchronize());
        XQ_TRY(alloc(count));
        if (grew) *grew = true;
        return XQ_OK;
    }
};
template <class T> using PinnedBuf = DevBuf<T, PinnedMem>;

}  // namespace xq

// replay ring in HBM: structure of arrays, states as packed boards (48 B) — never 1260 floats.  A plain view, passed to kernels by
// value; xq_replay owns the memory behind it.
struct ReplayDev {
    uint32_t* boards = nullptr;       // [capacity][12]
    uint32_t* next_boards = nullptr;  // [capacity][12]
    int32_t* action_to = nullptr;     // [capacity]   action.to (0..89), -1 = empty slot (contributes no gradient)
    float* reward = nullptr;          // [capacity]
    uint8_t* done = nullptr;          // [capacity]
    uint8_t* next_player = nullptr;   // [capacity]   side to move in next_boards (0 Red, 1 Black); nullptr until xq_replay_track_next_player
    uint8_t* mover = nullptr;         // [capacity]   side that moved in `boards` (the learner's colour in versus training); nullptr until xq_replay_track_mover
    int capacity = 0;
    // prioritized replay (xq_replay_enable_per; nullptr = uniform): priority of every slot = leaves of the sum tree, and the
    // largest priority assigned so far as it stood at the last rebuild (what a new transition enters with), as float bits
    float* prio = nullptr;            // [capacity rounded up to 32]
    const unsigned* pmax_snap = nullptr;
};

struct xq_replay {
    ReplayDev dev;
    xq::DevBuf<uint32_t> boards, next_boards;     // what `dev` points into
    xq::DevBuf<int32_t> action_to;
    xq::DevBuf<float> reward, prio;
    xq::DevBuf<uint8_t> done, next_player, mover;
    int size = 0;
    int write_pos = 0;
    uint64_t total = 0;
    uint64_t seed = 0;
    uint64_t sample_calls = 0;
    xq::DevBuf<int32_t> slots_dev;    // last sample()
    int last_batch = 0;
    bool implicit = false;            // last sample() was "virtual": consumers derive slot i = philox(i, call) % size themselves
    uint32_t implicit_call = 0;
    int implicit_size = 0;
    int implicit_start = 0;           // windowed sample: slot = (start + philox % size) % capacity
    // n-step returns (xq_replay_set_n_step, DESIGN.md §4 "n-step returns"): chain length (1 = off) and the distance in age order between
    // successive transitions of one trajectory; read_first / read_count: the readable range of the NEXT xq_dqn_td_grads_replay when its
    // owner narrowed it (replay_set_readable; read_count < 0: the default — the filled ring in age order), consumed by that step
    int n_step = 1, n_stride = 1;
    int read_first = 0, read_count = -1;
    // mirror augmentation (xq_replay_set_mirror, DESIGN.md §4 "Mirror augmentation"): the probability that a minibatch row is reflected
    // left-right in the staged batch (0 = off), and the number of mirror-mode TD steps queued from this ring so far — the `call` word of
    // the next one's flag stream
    double mirror_prob = 0.0;
    uint64_t mirror_calls = 0;
    // colour-swap augmentation (xq_replay_set_colour_swap, DESIGN.md §4 "Colour-swap augmentation"): the same pair for the exchange of
    // the colours with row -> 9 - row; a counter of its own (the mirror's is untouched)
    double colour_swap_prob = 0.0;
    uint64_t colour_swap_calls = 0;
    xq::Stream stream;
    // Device data of the ring that other handles read or write, possibly on streams of their own — each a SharedResource (above):
    //   contents : boards / next_boards / action_to / reward / done   written by env steps (xq_env_selfplay_step) and push_host,
    //              read by TD steps (xq_dqn_td_grads_replay)
    //   prio     : live priority table + running maximum, and the tree / snapshot a rebuild makes of them
    //              written by env steps (new transitions enter with the snapshot maximum), by TD steps (TD-error priorities) and by
    //              a rebuild; every one of them also reads what the one before wrote, so they are all writers.  (Draws read the tree on
    //              the stream the rebuild ran on — the ring's — and need no entry.)
    //   draw     : slot list, importance weights, batch maximum          written by a draw, read by the TD step that consumes it
    // Every access goes through read() / write(), which order the accessing stream behind the accesses it depends on when those ran
    // on another stream; on one stream (the trainer's layout) they cost nothing.  `caller_orders`: the owner orders the accesses
    // itself (xq_trainer: its collects write ring slots that the TD step running beside them never samples).
    xq::SharedResource contents{xq::ORD_RING_CONTENTS}, prio_res{xq::ORD_RING_PRIORITIES}, draw{xq::ORD_RING_DRAW};
    bool caller_orders = false;
    // prioritized replay (build-defined, BASELINE configs[4]): radix-32 sum tree, level 0 = dev.prio
    struct Per {
        bool enabled = false;
        float alpha = 0.6f, beta = 0.4f, eps = 1e-3f;
        int nlv = 0, n[8] = {0}, p[8] = {0};
        xq::DevBuf<float> leaves;        // level 0 as of the last rebuild (copy of dev.prio; the sampler reads this, never the live table)
        xq::DevBuf<float> upper;         // levels 1.. concatenated (padded), root last
        size_t off[8] = {0};              // offset of level lv inside `upper` (lv >= 1)
        xq::DevBuf<unsigned> scalars;    // [0] max priority, live (atomicMax of float bits)  [1] its snapshot at the last rebuild
                                          // [2] max raw importance weight of the last sample (float bits)  [3] eligible slots (p > 0)
        xq::DevBuf<unsigned> wave_counts;  // per-wave counts of non-zero leaves of the last rebuild (summed into scalars[3] by per_upper_kernel)
        bool wmax_clean = false;          // scalars[2] is zero (set by a rebuild, consumed by the next draw)
        bool draw_unconsumed = false;     // a prioritized draw whose TD step has not been queued yet: a rebuild must leave scalars[2] alone
        xq::DevBuf<float> is_w;          // [slots_dev.n] raw importance weights of the last prioritized sample
        bool last_prioritized = false;
    } per;
};

struct xq_env {
    int n = 0;
    uint64_t seed = 0;
    uint32_t first_id = 0;
    xq::Stream stream;
    xq::DevBuf<uint32_t> boards;       // [n][12]
    xq::DevBuf<uint4> meta;            // [n] {moveCount|player<<16, red|black<<16, plies, episodes}
    xq::DevBuf<uint4> stats;           // [n] {red wins, black wins, captures, explored}
    xq::DevBuf<xq_step_result> results; // [n]
    xq::DevBuf<uint16_t> codes;        // [n][128] scratch for legal_moves
    xq::DevBuf<int32_t> counts;        // [n]
    xq::DevBuf<int32_t> actions;       // [n] scratch for step()
    xq::DevBuf<float> q90;             // [n][96] scratch for selfplay_step_host
    xq::DevBuf<uint8_t> validmat;      // [8100]
    xq::DevBuf<xq_episode_record> ep_ring;
    int ep_cap = 0;
    xq::DevBuf<unsigned long long> ep_head;  // device counter of finished episodes
    uint64_t ep_drained = 0;
    // the reward the env kernel writes into a ring (xq_env_set_reward), as given; the launches carry the fp32 values
    int rw_kind = XQ_REWARD_EVALUATE;
    double rw_scale = 1e-3, rw_cost = 0.0, rw_bound = 1.0;
    // the Q rows handed to the self-play and versus-learner launches are in the mover's view (xq_env_set_q_view)
    int q_view = 0;
    // how a ply that reads Q rows and did not explore picks its move (xq_env_set_policy); GREEDY keeps the last temperature unused
    int policy_kind = XQ_POLICY_GREEDY;
    double temperature = 1.0;
};

namespace xq {

// HIP-event profiler: brackets individual launches on the handle's stream (bench.py roofline leg).  Disabled = free.
struct Profiler {
    struct Cat { char name[48]; double flops = 0, bytes = 0; int launches = 0; int exact = 0; float ms = 0; };   // exact: launches timed by their own events
    struct Rec { int cat; Event a, b; bool attached; };   // attached: a / b are the start / stop events of the kernel's own launch
    struct Span { char name[48]; float start_ms, end_ms; };      // relative to the first bracket of the batch (live timeline)
    std::vector<Span> spans;
    bool enabled = false;
    bool roofline_only = false;   // bracket only the kernels named in `only` (keeps the timed region undisturbed)
    int sample_period = 1;        // roofline_only: bracket every sample_period-th launch of a named kernel (an event record drains
                                  // the recording queue: ~10 us per bracket on a stream of 10-50 us kernels, tools/sync_probe.hip)
    struct Only { char name[48]; int phase; int period_add; };
    std::vector<Only> only;       // xq_dqn_kernel_filter; default = the three kernels bench.py priced in rounds 1-3
    void set_only(const char* csv) {
        only.clear();
        for (const char* p = csv; p && *p;) {
            const char* q = strchr(p, ',');
            const size_t len = q ? (size_t)(q - p) : strlen(p);
            Only o; memset(&o, 0, sizeof o);
            memcpy(o.name, p, len < sizeof o.name - 1 ? len : sizeof o.name - 1);
            // the env kernel on a period of its own, sample_period + 1: with 4 plies per update a shared period of 4 would always
            // pick the same ply
            o.period_add = strncmp(o.name, "env_selfplay_step", 17) == 0 ? 1 : 0;
            if (len) only.push_back(o);
            p = q ? q + 1 : nullptr;
        }
    }
    std::vector<Cat> cats;
    std::vector<Rec> recs;
    std::vector<Event> pool;
    int cat_id(const char* name) {
        for (size_t i = 0; i < cats.size(); ++i) if (!strcmp(cats[i].name, name)) return (int)i;
        Cat c; memset(c.name, 0, sizeof c.name); strncpy(c.name, name, sizeof c.name - 1);
        cats.push_back(c);
        return (int)cats.size() - 1;
    }
    int get_event(Event* e) {
        if (pool.empty()) return e->create(hipEventDefault);
        *e = std::move(pool.back()); pool.pop_back();
        return XQ_OK;
    }
    // attach: the caller hands recs[h].a / .b to hipExtLaunchKernelGGL as the launch's start / stop events — the elapsed time is then the
    // kernel's own (what rocprofv3 reports), with no marker packets on the stream; otherwise the pair is recorded around the scope
    // (one or more launches; reads ~6.5 us more than a single kernel, tools/sync_probe.hip)
    int begin(const char* name, hipStream_t s, bool attach = false) {
        if (!enabled) return -1;
        if (roofline_only) {
            if (only.empty()) set_only("gemm_qmax_rowmax,gemm_qmax_screen,env_selfplay_step");
            Only* o = nullptr;
            for (auto& x : only) if (!strcmp(x.name, name)) { o = &x; break; }
            if (!o) return -1;
            const int period = sample_period > 1 ? sample_period + o->period_add : 1;
            if (period > 1 && (o->phase++ % period) != 0) return -1;
        }
        Rec r;
        if (get_event(&r.a) != XQ_OK || get_event(&r.b) != XQ_OK) return -1;     // no events: this launch is not bracketed
        r.cat = cat_id(name); r.attached = attach;
        if (!attach) (void)hipEventRecord(r.a, s);
        recs.push_back(std::move(r));
        return (int)recs.size() - 1;
    }
    void end(int h, hipStream_t s, double flops, double bytes) {
        if (h < 0) return;
        if (!recs[h].attached) (void)hipEventRecord(recs[h].b, s);
        Cat& c = cats[recs[h].cat];
        c.flops += flops; c.bytes += bytes; c.launches += 1; c.exact += recs[h].attached ? 1 : 0;
    }
    void collect() {
        if (!recs.empty()) spans.clear();
        for (auto& r : recs) {
            float ms = 0;
            (void)hipEventSynchronize(r.b);
            (void)hipEventElapsedTime(&ms, r.a, r.b);
            cats[r.cat].ms += ms;
            if (!roofline_only && spans.size() < 8192) {
                Span sp; memcpy(sp.name, cats[r.cat].name, sizeof sp.name); sp.start_ms = 0; sp.end_ms = 0;
                (void)hipEventElapsedTime(&sp.start_ms, recs[0].a, r.a);
                (void)hipEventElapsedTime(&sp.end_ms, recs[0].a, r.b);
                spans.push_back(sp);
            }
        }
        for (auto& r : recs) { pool.push_back(std::move(r.a)); pool.push_back(std::move(r.b)); }
        recs.clear();
    }
    void reset() { collect(); cats.clear(); }
    ~Profiler() { collect(); }
};
struct ProfilerOff {                  // while one lives, the profiler brackets nothing
    Profiler& p; bool was;
    explicit ProfilerOff(Profiler* q) : p(*q), was(q->enabled) { p.enabled = false; }
    ~ProfilerOff() { p.enabled = was; }
};

// communicator internals (xq_comm.hip)
int comm_allreduce_on(xq_comm* c, float* buf, size_t n_floats, hipStream_t stream);   // in-place sum over all ranks
int comm_world(const xq_comm* c);

// dqn-side entry points used by the trainer (defined in xq_dqn.hip)
Profiler* dqn_profiler(xq_dqn* d);
xq_comm* dqn_comm(const xq_dqn* d);         // communicator attached with xq_dqn_set_comm, or nullptr
int dqn_fused_apply(const xq_dqn* d);      // current xq_dqn_set_fused_apply setting
// Q[0..95] of the select chain still as the k-slabs of the head ([nslabs][n][96], nslabs even): the env kernel adds them, the bias and
// the tanh itself, for the boards that exploit (dqn_q90_boards fills it when the head rode on the last hidden product)
struct QSource { const float* slabs; long long slab_stride; int nslabs; const float* bias; };
// qs != nullptr: when the select head rides on the last hidden product, its k-slabs are handed over as they are (qs->slabs != nullptr,
// *q90_dev = nullptr) for the env kernel to finish; otherwise qs->slabs = nullptr and *q90_dev holds the finished values as always
int dqn_q90_boards(xq_dqn* d, const uint32_t* boards_dev, int n, float** q90_dev, int* q_stride, hipStream_t on = nullptr, QSource* qs = nullptr);
hipStream_t dqn_stream(xq_dqn* d);
int dqn_view(const xq_dqn* d);              // current xq_dqn_set_view setting
// view_boards_kernel (xq_stage.hip.h) on `stream`: out[b] = view(boards[b], side of b), the side from side_dev[b] or, with meta_dev (an
// env's boards), from bit 16 of meta_dev[b].x
int view_boards_launch(const uint32_t* boards_dev, const uint8_t* side_dev, const uint4* meta_dev, int n, uint32_t* out_dev, hipStream_t stream);
hipEvent_t dqn_qmax_event(xq_dqn* d);      // recorded behind the column-max GEMM of the last xq_dqn_td_grads*
uint64_t dqn_params_version(const xq_dqn* d);   // counts the operations that rewrote parameters (either net, fp32 or the bf16 shadow)

// "virtual" replay sample: same slots as xq_replay_sample would write (Philox ctr = {i, 0, call, 1}, key = seed, % size),
// but no kernel and no slot buffer — the consumer kernels recompute them.  Used by the trainer's hot loop.
// (start, count) restricts the draw to `count` ring slots from `start` (count < 0: the whole filled part).
int replay_sample_implicit(xq_replay* r, int batch, int start = 0, int count = -1);

// cross-stream ordering of the ring's users (SharedResource; no-ops on one stream or when the owner orders: xq_replay::caller_orders)
int replay_consumer_begin(xq_replay* r, hipStream_t consumer, bool listed, bool prioritized);   // a TD step that reads the ring
int replay_writer_begin(xq_replay* r, hipStream_t writer);                                      // an env step that writes it
void replay_advance(xq_replay* r, int n);   // n transitions were written (or queued) from write_pos on: moves write_pos, size and total
// prioritized replay internals used by the trainer (xq_replay.hip)
// hold: `hold_count` slots from `hold_start` (wrapping) count as priority 0 in the snapshot and the sums only (n-step returns: slots whose
// chains are not complete yet); the live table keeps their values
int replay_per_rebuild(xq_replay* r, int retire_start, int retire_count, hipStream_t on, int hold_start = 0, int hold_count = 0);
// the readable range of the next n-step TD step from this ring: `count` slots in age order from slot `first` (count < 0: the default)
void replay_set_readable(xq_replay* r, int first, int count);
inline RingState ring_state(const xq_replay* r) { return {r->size, r->write_pos, r->dev.capacity}; }
int replay_per_sample(xq_replay* r, int batch, hipStream_t on);

// env-side launchers used by the trainer
int env_selfplay_launch(xq_env* env, const float* q90_dev, int q_stride, uint32_t eps_u32, xq_step_result* results_dev,
                        xq_replay* replay, hipStream_t on = nullptr, const QSource* qs = nullptr, hipEvent_t ev_start = nullptr,
                        hipEvent_t ev_stop = nullptr);      // ev_*: the kernel's own start / stop events (profiler, kernel-exact timing)
int env_arena_launch(xq_env* env, const float* q90_dev, int q_stride, int pairs, int opening, const uint32_t eps_u32[2],
                     const int has_q[2], xq_arena_game* records_dev, int* live_dev, xq_step_result* results_dev,
                     const int16_t* pick_dev, const int pick_on[2], const int q_view[2] = nullptr,    // xq_arena.hip; q_view: per half, the
                     const float inv_temp[2] = nullptr);                                              // rows are in the mover's view;
                                                                                                     // inv_temp: per half, 0 = greedy
void dqn_shape(const xq_dqn* d, int* n_in, int* n_out);    // layer_sizes[0], outputs
constexpr uint32_t kMetaFrozen = 1u << 20;                  // meta.x flag of a finished arena game (xq_env.hip META_FROZEN)
constexpr uint32_t kMetaVsDone = 1u << 21;                  // meta.x flag: the game's versus slot of this collect is written (META_VS_DONE)
// versus training (xq_trainer_set_opponent): one phase of the collect, see env_versus_launch in xq_env.hip
int env_versus_launch(xq_env* env, int phase, const float* q90_dev, int q_stride, const QSource* qs, uint32_t eps_u32,
                      const int16_t* pick_dev, uint4* counts_dev, xq_replay* replay, hipStream_t on, int opponent_view = 0);
                      // (phase 1 reads the learner's rows by the env's q_view; opponent_view: phases 0 and 2, a net opponent's rows)
// The search player's picks (xq_search.hip) of games [first, first + count) of env, on stream s: pick_dev[g] = an index into game g's
// move list.  Arena: ties are broken on the stream of the pair (twin g - pairs).  seated (versus training, pairs = INT_MAX): only the
// games where the learner's opponent is to move, ties on the game's own stream.
int search_pick_launch(xq_env* env, int depth, int first, int count, int pairs, bool seated, uint32_t eps_u32, int16_t* pick_dev,
                       hipStream_t s);

// ---- a player that moves on an env: the arena's two sides and the trainer's opponent (defined in xq_arena.hip) ----------------------
// floor(eps * 2^32), saturated: the threshold the env kernel holds a Philox word against (vecenv.eps_to_u32 is the Python mirror)
inline uint32_t eps_to_u32(double eps) { return (uint32_t)std::min(std::max(eps, 0.0) * 4294967296.0, 4294967295.0); }
// A Boltzmann temperature (xq_env_set_policy, xq_arena_set_temperature) is held on its fp32 value: finite and in [1e-3, 1e3]; every
// comparison is false for a NaN.  The kernel takes (float)(1 / T), formed in double
inline bool temperature_ok(double t) { const float f = (float)t; return f >= 1e-3f && f <= 1e3f; }
inline float temperature_to_inv(double t) { return (float)(1.0 / t); }
struct CheckedPlayer {
    int kind = XQ_PLAYER_RANDOM;
    xq_dqn* net = nullptr;      // XQ_PLAYER_NET: borrowed
    int depth = 0;              // XQ_PLAYER_SEARCH: 1..3
    uint32_t eps_u32 = 0;       // (0 for random play: every move explores anyway)
    int n_out = 96;             // XQ_PLAYER_NET: the Q columns to compute, min(outputs, 96)
    int view = 0;               // XQ_PLAYER_NET: the net reads the mover's view (its handle's xq_dqn_set_view when the player was made)
};
// in == nullptr: uniform-random play.  `who` opens the message of a rejected player ("xq_arena_run_players: player A")
int make_player(const xq_arena_player* in, const char* who, CheckedPlayer* out);
// Q rows [n][96] of n boards through the borrowed network d, on d's own stream: behind ev_env, which the caller has recorded on the
// consumer stream s behind the env's last launch, and ahead of whatever s queues next (ev_q; neither event is touched when d runs on
// s).  The forward keeps no layer-0 sums, touches no TD-step state and stays out of the handle's kernel statistics, so a lent network
// has the same bits afterwards.
int borrowed_forward(xq_dqn* d, const uint32_t* boards_dev, int n, int n_out, float* q_rows_dev, hipStream_t s, hipEvent_t ev_env,
                     hipEvent_t ev_q);
inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
}  // namespace xq
