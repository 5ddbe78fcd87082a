"""DQN / Trainer — host-side mirror of the reference's DQN (include/dqn.h:97-116) and ChessAI::train
(src/chessai.cpp:85-170) over the C ABI.  Same method names and argument meaning as upstream; all arithmetic
runs in libxqhip.so on the GPU (fp32 MFMA), fp64 at the boundary like upstream's std::vector<double>.
"""
import ctypes as C
import random

import numpy as np

from . import _capi
from ._capi import call, KernelStat, KernelSpan, TrainerConfig as _CConfig
from .vecenv import VecEnv, ReplayBuffer, _ptr, reward_kind, policy_kind
from .arena import Search, player

REFERENCE_LAYERS = (1260, 128, 8100)     # ChessAI::initializeDQN, chessai.cpp:395-404


class DQN:
    def __init__(self, layer_sizes=REFERENCE_LAYERS, learning_rate=0.001, gamma=0.99, seed=1, stream=None, _handle=None):
        self.layer_sizes = tuple(int(x) for x in layer_sizes)
        self.learning_rate, self.gamma = float(learning_rate), float(gamma)
        self._own = _handle is None
        if _handle is None:
            sizes = (C.c_int32 * len(self.layer_sizes))(*self.layer_sizes)
            h = C.c_void_p()
            call("xq_dqn_create", sizes, len(self.layer_sizes), self.learning_rate, self.gamma, int(seed), stream,
                 C.byref(h))
            _handle = h
        self._h = _handle
        nw, nb = C.c_size_t(), C.c_size_t()
        call("xq_dqn_num_params", self._h, C.byref(nw), C.byref(nb))
        self.n_weights, self.n_biases = nw.value, nb.value
        self._rng = random.Random(seed)

    def close(self):
        if self._h is not None and self._own:
            call("xq_dqn_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def stream(self):
        s = C.c_void_p()
        call("xq_dqn_stream", self._h, C.byref(s))
        return s.value

    # ---- parameters in the reference flat layout (host_weights / host_biases, dqn.h:47-50) ----
    def set_params(self, weights, biases, net=_capi.NET_ONLINE):
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(self.n_weights)
        b = np.ascontiguousarray(biases, dtype=np.float64).reshape(self.n_biases)
        call("xq_dqn_set_params", self._h, int(net), _ptr(w, C.c_double), _ptr(b, C.c_double))

    def get_params(self, net=_capi.NET_ONLINE):
        w = np.zeros(self.n_weights, dtype=np.float64)
        b = np.zeros(self.n_biases, dtype=np.float64)
        call("xq_dqn_get_params", self._h, int(net), _ptr(w, C.c_double), _ptr(b, C.c_double))
        return w, b

    # ---- DQN API (dqn.h:102-109) ----
    def getQValues(self, state, net=_capi.NET_ONLINE):
        """state: [L0] or [n][L0] doubles -> [nout] or [n][nout]."""
        x = np.ascontiguousarray(state, dtype=np.float64)
        single = x.ndim == 1
        x = x.reshape(-1, self.layer_sizes[0])
        q = np.zeros((len(x), self.layer_sizes[-1]), dtype=np.float64)
        call("xq_dqn_forward", self._h, int(net), _ptr(x, C.c_double), len(x), _ptr(q, C.c_double))
        return q[0] if single else q

    def selectAction(self, state, epsilon, valid_actions, rand1=None, rand2=None):
        """DQN::selectAction (dqn.cpp:24-56).  valid_actions: sequence of (from, to).  rand1 in [0,1) and rand2
        (non-negative int) replace the two rand() draws when given (parity tests inject them)."""
        if len(valid_actions) == 0:
            raise RuntimeError("No valid actions available.")
        r1 = self._rng.random() if rand1 is None else rand1
        if r1 < epsilon:
            r2 = self._rng.randrange(1 << 31) if rand2 is None else rand2
            return valid_actions[r2 % len(valid_actions)]
        q = self.getQValues(state)
        best, maxq = valid_actions[0], -np.inf
        for a in valid_actions:
            if a[1] >= len(q):
                continue
            if q[a[1]] > maxq:
                maxq, best = q[a[1]], a
        return best

    def backpropagate(self, state, target, learning_rate=None, grad_scale=1.0, mode=_capi.BACKPROP_REFERENCE):
        x = np.ascontiguousarray(state, dtype=np.float64).reshape(-1, self.layer_sizes[0])
        t = np.ascontiguousarray(target, dtype=np.float64).reshape(-1, self.layer_sizes[-1])
        assert len(x) == len(t)
        lr = self.learning_rate if learning_rate is None else learning_rate
        call("xq_dqn_backpropagate", self._h, _ptr(x, C.c_double), _ptr(t, C.c_double), len(x), float(lr),
             float(grad_scale), int(mode))

    def updateTargetNetwork(self, tau=None):
        """DQN::updateTargetNetwork (dqn.cpp:71-74): the whole copy; with tau, one soft update of the whole target net now
        (theta- += tau (theta - theta-); tau = 1 is the copy, tau = 0 a no-op), whatever set_target_tau says."""
        if tau is None:
            call("xq_dqn_update_target", self._h)
        else:
            call("xq_dqn_soft_update_target", self._h, _checked_tau("updateTargetNetwork", tau))

    def saveModel(self, filename):
        call("xq_dqn_save_model", self._h, str(filename).encode())

    def loadModel(self, filename):
        call("xq_dqn_load_model", self._h, str(filename).encode())

    def train(self, state, action, reward, next_state, done, mode=_capi.BACKPROP_REFERENCE):
        """DQN::train (dqn.cpp:157-172): single transition, target network for max Q(s').  The reference's rule only: under
        set_zero_sum(True) it raises ValueError (the zero-sum target lives in the batched TD step)."""
        if hasattr(_capi.load(), "xq_dqn_get_view") and self.view() == "mover":
            raise ValueError("DQN.train reads absolute boards on the host; the mover view (set_view) is the batched paths': build the "
                             "view with view_boards and use td_update, or td_grads_replay from a tracking ring")
        if hasattr(_capi.load(), "xq_dqn_get_zero_sum") and self.zero_sum():
            raise ValueError("DQN.train forms the reference's target r + gamma max Q(s') on the host; the zero-sum target "
                             "(set_zero_sum) is the batched TD step's: use td_update / td_grads_replay / Trainer")
        q = self.getQValues(state)
        if done:
            q[action] = reward
        else:
            q[action] = reward + self.gamma * self.getQValues(next_state, net=_capi.NET_TARGET).max()
        self.backpropagate(state, q, self.learning_rate, 1.0, mode)

    # ---- batched device-side TD step on packed boards ----
    def td_update(self, boards, next_boards, action_to, reward, done, td_net=_capi.TD_ONLINE_NET,
                  mode=_capi.BACKPROP_REFERENCE, learning_rate=None, grad_scale=1.0, next_player=None):
        """One TD update on host transitions; returns (Q(s,a), y).  next_player: the side to move in each next board (0 = Red,
        1 = Black) — what set_td_bootstrap("legal") needs; without it the unsided entry point is called."""
        b = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 90)
        nb = np.ascontiguousarray(next_boards, dtype=np.uint8).reshape(-1, 90)
        n = len(b)
        a = np.ascontiguousarray(action_to, dtype=np.int32).reshape(n)
        r = np.ascontiguousarray(reward, dtype=np.float32).reshape(n)
        d = np.ascontiguousarray(done, dtype=np.uint8).reshape(n)
        qsa, y = np.zeros(n, np.float32), np.zeros(n, np.float32)
        lr = self.learning_rate if learning_rate is None else learning_rate
        if next_player is not None:
            p = np.ascontiguousarray(next_player, dtype=np.uint8).reshape(n)
            call("xq_dqn_td_update_host_sided", self._h, n, _ptr(b, C.c_uint8), _ptr(nb, C.c_uint8), _ptr(a, C.c_int32),
                 _ptr(r, C.c_float), _ptr(d, C.c_uint8), _ptr(p, C.c_uint8), int(td_net), int(mode), float(lr), float(grad_scale),
                 _ptr(qsa, C.c_float), _ptr(y, C.c_float))
            return qsa, y
        call("xq_dqn_td_update_host", self._h, n, _ptr(b, C.c_uint8), _ptr(nb, C.c_uint8), _ptr(a, C.c_int32),
             _ptr(r, C.c_float), _ptr(d, C.c_uint8), int(td_net), int(mode), float(lr), float(grad_scale),
             _ptr(qsa, C.c_float), _ptr(y, C.c_float))
        return qsa, y

    def q_boards(self, env, n_out=96, net=_capi.NET_ONLINE):
        """Q-values of the first n_out outputs for every board of a VecEnv (device -> host copy via torch-free path)."""
        import torch
        q = torch.empty((env.n_games, n_out), dtype=torch.float32, device="cuda")
        call("xq_dqn_forward_boards_dev", self._h, int(net), C.c_void_p(env.boards_dev()), env.n_games, int(n_out),
             C.c_void_p(q.data_ptr()), int(n_out))
        call("xq_stream_synchronize", None)
        torch.cuda.synchronize()
        return q

    def select_q(self, env):
        """Q(s)[0..95] of every board of a VecEnv through the select chain of the self-play loop (xq_dqn_select_q_dev)."""
        import torch
        q = torch.empty((env.n_games, 96), dtype=torch.float32, device="cuda")
        call("xq_dqn_select_q_dev", self._h, C.c_void_p(env.boards_dev()), env.n_games, C.c_void_p(q.data_ptr()))
        call("xq_stream_synchronize", None)
        torch.cuda.synchronize()
        return q

    def td_grads_replay(self, replay, batch, td_net=_capi.TD_ONLINE_NET, mode=_capi.BACKPROP_REFERENCE):
        """Gradients of one TD minibatch taken from a replay ring (batch = 0: the whole filled ring, in order)."""
        call("xq_dqn_td_grads_replay", self._h, replay.handle, int(batch), int(td_net), int(mode))

    def apply_grads(self, learning_rate=None, grad_scale=1.0):
        lr = self.learning_rate if learning_rate is None else learning_rate
        call("xq_dqn_apply_grads", self._h, float(lr), float(grad_scale))

    def grad_buffer(self):
        p, n = C.c_void_p(), C.c_size_t()
        call("xq_dqn_grad_buffer", self._h, C.byref(p), C.byref(n))
        return p.value, n.value

    def last_loss(self):
        v = C.c_double()
        call("xq_dqn_last_loss", self._h, C.byref(v))
        return v.value

    def last_td_values(self, n):
        """(Q(s,a), y) of the first n samples of the last TD step."""
        q, y = np.zeros(n, np.float32), np.zeros(n, np.float32)
        call("xq_dqn_last_td_values", self._h, int(n), _ptr(q, C.c_float), _ptr(y, C.c_float))
        return q, y

    def last_n_step(self, n):
        """The first n rows of the batch the last td_grads_replay assembled from a ring with n_step > 1: dict of reward (the n-step R),
        done, steps (chain elements used), first_slot (the sampled slot), last_slot (whose next board was staged) and action (-1: a
        dead row).  Raises XqError when the last TD step was not an n-step one."""
        r, d = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        m, f, l, a = (np.zeros(n, np.int32) for _ in range(4))
        call("xq_dqn_last_n_step", self._h, int(n), _ptr(r, C.c_float), _ptr(d, C.c_uint8), _ptr(m, C.c_int32), _ptr(f, C.c_int32),
             _ptr(l, C.c_int32), _ptr(a, C.c_int32))
        return dict(reward=r, done=d, steps=m, first_slot=f, last_slot=l, action=a)

    def last_mirror(self, n):
        """The first n rows of the batch the last td_grads_replay staged from a ring with ReplayBuffer.set_mirror(prob > 0): dict of
        flags (1 = the row was reflected), boards and next_boards ([n, 90] piece codes as staged), action (as staged) and slot (the
        sampled slot).  Raises XqError when the last TD step was not a mirror-mode one."""
        f, out, (b, nb, a, s) = np.zeros(n, np.uint8), *_staged_rows(n)
        call("xq_dqn_last_mirror", self._h, int(n), _ptr(f, C.c_uint8), b, nb, a, s)
        return dict(flags=f, **out)

    def last_colour_swap(self, n, next_player=False):
        """The first n rows of the batch the last td_grads_replay staged from a ring with ReplayBuffer.set_colour_swap(prob > 0): dict
        of flags (1 = the row's colours were exchanged), boards and next_boards ([n, 90] piece codes as staged), action (as staged) and
        slot (the sampled slot); with next_player=True also next_player (the staged side bytes: only behind a step under the legal-move
        bootstrap).  With the mirror on as well this is the same staged batch last_mirror reports, with this transform's flags.  Raises
        XqError when the last TD step was not a colour-swap-mode one."""
        f, out, (b, nb, a, s) = np.zeros(n, np.uint8), *_staged_rows(n)
        p = np.zeros(n, np.uint8) if next_player else None
        call("xq_dqn_last_colour_swap", self._h, int(n), _ptr(f, C.c_uint8), b, nb, a, _ptr(p, C.c_uint8) if next_player else None, s)
        out = dict(flags=f, **out)
        if next_player:
            out["next_player"] = p
        return out

    def last_view(self, n):
        """The first n rows of the batch the last td_grads_replay staged under set_view("mover"): dict of flag_s (1 = Black moved: s and
        the action were swapped), flag_next (1 = Black moves next: s' was swapped), boards and next_boards ([n, 90] piece codes as
        staged), action (as staged) and slot (the sampled slot).  Raises XqError when the last TD step was not a view-mode one."""
        f, fn, out, (b, nb, a, s) = np.zeros(n, np.uint8), np.zeros(n, np.uint8), *_staged_rows(n)
        call("xq_dqn_last_view", self._h, int(n), _ptr(f, C.c_uint8), _ptr(fn, C.c_uint8), b, nb, a, s)
        return dict(flag_s=f, flag_next=fn, **out)

    def kernel_stats(self, enable=-1):
        """Returns the HIP-event timings collected so far; enable: 1 on, 0 off, 2 on + clear, -1 leave."""
        arr = (KernelStat * 64)()
        n = C.c_int32()
        call("xq_dqn_kernel_stats", self._h, int(enable), arr, 64, C.byref(n))
        return [dict(name=arr[i].name.decode(), ms=arr[i].ms, launches=arr[i].launches, flops=arr[i].flops,
                     bytes=arr[i].bytes, exact=arr[i].exact_launches) for i in range(n.value)]


def _staged_rows(n):
    """What every staging transform's read-back returns for n rows: (dict of boards, next_boards, action, slot; their pointers in the
    C calls' order)"""
    out = dict(boards=np.zeros((n, 90), np.uint8), next_boards=np.zeros((n, 90), np.uint8), action=np.zeros(n, np.int32),
               slot=np.zeros(n, np.int32))
    return out, (_ptr(out["boards"], C.c_uint8), _ptr(out["next_boards"], C.c_uint8), _ptr(out["action"], C.c_int32),
                 _ptr(out["slot"], C.c_int32))


def _kernel_filter(self, names=None):
    """Which launches kernel_stats(enable=3 / 4) brackets: an iterable of bracket names (None = the default three)."""
    call("xq_dqn_kernel_filter", self._h, ",".join(names).encode() if names else None)


DQN.kernel_filter = _kernel_filter


def _set_precision(self, precision):
    """_capi.PRECISION_F32 / PRECISION_BF16: arithmetic of the forward passes on packed boards (bf16 MFMA Q-net)."""
    call("xq_dqn_set_precision", self._h, int(precision))


DQN.set_precision = _set_precision


def _set_qmax_mode(self, mode):
    """_capi.QMAX_FULL / QMAX_SCREENED: how the TD step finds max_a' Q(s', a') (exact bf16 screening + fp32 re-evaluation)."""
    call("xq_dqn_set_qmax_mode", self._h, int(mode))


def _set_l0_derive(self, on):
    """Layer-0 sums of s' derived from those of s (online TD rule, fp32 net): one gather instead of two, a different summation order."""
    call("xq_dqn_set_l0_derive", self._h, 1 if on else 0)


DQN.set_l0_derive = _set_l0_derive


def _set_td_tail(self, on):
    """Gradient half of a TD step as fused launches on one stream (default) or kernel by kernel on two streams; same bits."""
    call("xq_dqn_set_td_tail", self._h, 1 if on else 0)


DQN.set_td_tail = _set_td_tail


def _set_l0_grad_mode(self, mode):
    """Layer-0 weight gradient: 1 = exact dense product on the bf16 matrix pipe (library default, where the shape allows), 0 = segmented sums."""
    call("xq_dqn_set_l0_grad_mode", self._h, int(mode))


DQN.set_l0_grad_mode = _set_l0_grad_mode


def _set_refine_stage(self, mode):
    """Exact screening, whole groups that many samples of a block share: -1 = through LDS while the screen's counters show many of them (default),
    0 = never, 1 = whenever the launch has room.  Same bits either way."""
    call("xq_dqn_set_refine_stage", self._h, int(mode))


DQN.set_refine_stage = _set_refine_stage


def _set_exchange_overlap(self, mode):
    """Data-parallel step: -1 auto, 0 select chain beside the gradient kernels, 1 beside the all-reduce (hides the exchange)."""
    call("xq_dqn_set_exchange_overlap", self._h, int(mode))


DQN.set_exchange_overlap = _set_exchange_overlap


def _calibrate_exchange(self, threshold_us=-1.0):
    """COLLECTIVE: time 20 all-reduces of the gradient buffer on the attached communicator; the auto setting of set_exchange_overlap
    then starts the select chain late iff their mean over the ranks exceeds threshold_us (< 0: the library's 41 us)."""
    us, late = C.c_double(0.0), C.c_int(0)
    call("xq_dqn_calibrate_exchange", self._h, float(threshold_us), C.byref(us), C.byref(late))
    return {"allreduce_us": us.value, "late_start": bool(late.value)}


def _exchange_calibration(self):
    """what the last calibration (explicit, or xq_dqn_set_comm's with more than one rank) measured and chose; None: none yet"""
    cal, late, us, thr = C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    call("xq_dqn_exchange_calibration", self._h, C.byref(cal), C.byref(us), C.byref(thr), C.byref(late))
    if not cal.value:
        return None
    return {"allreduce_us": us.value, "threshold_us": thr.value, "late_start": bool(late.value),
            "rule": "select chain starts behind the gradient kernels (beside the all-reduce) iff the measured all-reduce exceeds the threshold"}


DQN.calibrate_exchange = _calibrate_exchange
DQN.exchange_calibration = _exchange_calibration


def _qmax_stats(self):
    """(TD steps screened, samples, candidate (sample, group) pairs, pairs re-evaluated as whole groups); synchronises."""
    st = (C.c_uint64 * 4)()
    call("xq_dqn_qmax_stats", self._h, st)
    return tuple(int(x) for x in st)


def _qmax_guard(self):
    """(fallbacks to the full product so far, TD steps of the current fallback still to run)."""
    f, h = C.c_uint64(), C.c_int32()
    call("xq_dqn_qmax_guard", self._h, C.byref(f), C.byref(h))
    return f.value, h.value


DQN.set_qmax_mode = _set_qmax_mode
DQN.qmax_stats = _qmax_stats
DQN.qmax_guard = _qmax_guard


def _set_comm(self, comm):
    """Attach an xq_comm (dist.Comm) or None: td_grads then all-reduces the gradient buffer itself."""
    call("xq_dqn_set_comm", self._h, comm.handle if comm is not None else None)


DQN.set_comm = _set_comm


def _set_fused_apply(self, on=True):
    """apply_grads sums the layer-0 gradient partials itself (single GPU: nothing reads the gradient buffer in between)."""
    call("xq_dqn_set_fused_apply", self._h, 1 if on else 0)


DQN.set_fused_apply = _set_fused_apply


_OPT_KINDS = {"sgd": _capi.OPT_SGD, "adam": _capi.OPT_ADAM}


def _set_optimizer(self, kind="sgd", beta1=0.0, beta2=0.0, eps=0.0):
    """Optimizer of apply_grads / the trainer's learn_apply: "sgd" (default) or "adam" (torch.optim.Adam's rule, no weight decay;
    0 = the defaults 0.9 / 0.999 / 1e-8).  Changing the kind zeroes Adam's state.  backpropagate() stays plain SGD."""
    if kind not in _OPT_KINDS:
        raise ValueError(f"set_optimizer: expected 'sgd' or 'adam', got {kind!r}")
    call("xq_dqn_set_optimizer", self._h, _OPT_KINDS[kind], float(beta1), float(beta2), float(eps))


def _optimizer(self):
    """dict(kind, beta1, beta2, eps, steps): steps = Adam applies since the state was last reset."""
    k, t = C.c_int32(), C.c_uint64()
    b1, b2, e = C.c_double(), C.c_double(), C.c_double()
    call("xq_dqn_get_optimizer", self._h, C.byref(k), C.byref(b1), C.byref(b2), C.byref(e), C.byref(t))
    return dict(kind={v: n for n, v in _OPT_KINDS.items()}[k.value], beta1=b1.value, beta2=b2.value, eps=e.value, steps=t.value)


def _reset_optimizer(self):
    """Adam's m, v and step count back to 0."""
    call("xq_dqn_reset_optimizer", self._h)


def _optimizer_state(self):
    """(m, v, steps): Adam's moments as fp32 arrays in the layout of the gradient buffer; synchronises."""
    n = self.grad_buffer()[1]
    m, v, t = np.zeros(n, np.float32), np.zeros(n, np.float32), C.c_uint64()
    call("xq_dqn_get_optimizer_state", self._h, _ptr(m, C.c_float), _ptr(v, C.c_float), C.byref(t))
    return m, v, t.value


def _set_optimizer_state(self, m, v, steps):
    n = self.grad_buffer()[1]
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(n)
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(n)
    call("xq_dqn_set_optimizer_state", self._h, _ptr(m, C.c_float), _ptr(v, C.c_float), int(steps))


DQN.set_optimizer = _set_optimizer
DQN.optimizer = _optimizer
DQN.reset_optimizer = _reset_optimizer
DQN.optimizer_state = _optimizer_state
DQN.set_optimizer_state = _set_optimizer_state


def _set_grad_clip(self, max_norm):
    """Clip the gradient of apply_grads / the trainer's learn_apply by its global L2 norm (torch.nn.utils.clip_grad_norm_'s rule, in
    front of either optimizer): 0 = off (default), math.inf = measure the norm and never clip.  backpropagate() is never clipped."""
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"set_grad_clip: max_norm must be 0 (off), positive or inf, got {max_norm!r}")
    call("xq_dqn_set_grad_clip", self._h, max_norm)


def _grad_clip(self):
    """max_norm in force (0.0 = off)."""
    v = C.c_double()
    call("xq_dqn_get_grad_clip", self._h, C.byref(v))
    return v.value


def _grad_clip_stats(self):
    """dict(last_norm, last_coef, applies, clipped): norm and coefficient of the last clipped-mode apply; applies and how many of them
    had a coefficient below 1 since clipping was last switched on.  Synchronises; raises XqError while clipping is off."""
    n, c = C.c_double(), C.c_double()
    a, k = C.c_uint64(), C.c_uint64()
    call("xq_dqn_grad_clip_stats", self._h, C.byref(n), C.byref(c), C.byref(a), C.byref(k))
    return dict(last_norm=n.value, last_coef=c.value, applies=a.value, clipped=k.value)


DQN.set_grad_clip = _set_grad_clip
DQN.grad_clip = _grad_clip
DQN.grad_clip_stats = _grad_clip_stats


_LOSS_KINDS = {"squared": _capi.LOSS_SQUARED, "huber": _capi.LOSS_HUBER}


def _set_td_loss(self, kind="squared", kappa=1.0):
    """Loss of the TD step (td_grads* / the trainer's learn_grads): "squared" (default) or "huber" — the error e = Q(s,a) - y enters
    the output delta clamped to [-kappa, kappa] (Mnih et al. 2015), the importance weight multiplies behind the clamp and the priority
    written back stays that of the raw error.  kappa > 0 or math.inf; ignored for "squared".  backpropagate() is never affected."""
    if kind not in _LOSS_KINDS:
        raise ValueError(f"set_td_loss: expected 'squared' or 'huber', got {kind!r}")
    kappa = float(kappa)
    if kind == "huber" and not kappa > 0.0:
        raise ValueError(f"set_td_loss: kappa must be positive or inf, got {kappa!r}")
    call("xq_dqn_set_td_loss", self._h, _LOSS_KINDS[kind], kappa)


def _td_loss(self):
    """dict(kind, kappa): the loss in force and the last kappa given to "huber" (1.0 before the first)."""
    k, v = C.c_int32(), C.c_double()
    call("xq_dqn_get_td_loss", self._h, C.byref(k), C.byref(v))
    return dict(kind={v_: n for n, v_ in _LOSS_KINDS.items()}[k.value], kappa=v.value)


def _td_error_stats(self):
    """dict(live, mean_abs, max_abs, mean_loss, linear) of the TD errors e = Q(s,a) - y of the last TD step's live samples: linear =
    samples with |e| > kappa (0 under the squared loss), mean_loss under the loss in force.  One small kernel on request; synchronises;
    raises XqError before the first TD step."""
    n, k = C.c_uint64(), C.c_uint64()
    ma, mx, ml = C.c_double(), C.c_double(), C.c_double()
    call("xq_dqn_td_error_stats", self._h, C.byref(n), C.byref(ma), C.byref(mx), C.byref(ml), C.byref(k))
    return dict(live=n.value, mean_abs=ma.value, max_abs=mx.value, mean_loss=ml.value, linear=k.value)


DQN.set_td_loss = _set_td_loss
DQN.td_loss = _td_loss
DQN.td_error_stats = _td_error_stats


_BOOTSTRAPS = {"all": _capi.BOOTSTRAP_ALL, "legal": _capi.BOOTSTRAP_LEGAL}


def _set_td_bootstrap(self, kind="all"):
    """What the TD target bootstraps from: "all" (default) = the maximum over all outputs of the net, "legal" = the maximum over the
    moves the side to move can play in s' (the move the epsilon = 0 policy would play there; y = r where it has none).  "legal" needs
    the side to move per transition — td_update(..., next_player=...) — and an fp32 net; the unsided entry points and td_grads_replay from a ring without
    ReplayBuffer.track_next_player() raise XqError while it is in force (Trainer.set_td_bootstrap sets both up)."""
    if kind not in _BOOTSTRAPS:
        raise ValueError(f"set_td_bootstrap: expected 'all' or 'legal', got {kind!r}")
    call("xq_dqn_set_td_bootstrap", self._h, _BOOTSTRAPS[kind])


def _td_bootstrap(self):
    """"all" or "legal": the bootstrap in force."""
    k = C.c_int32()
    call("xq_dqn_get_td_bootstrap", self._h, C.byref(k))
    return {v: n for n, v in _BOOTSTRAPS.items()}[k.value]


def _last_legal(self, n, z96=True):
    """The first n rows of the last TD step if it ran under set_td_bootstrap("legal"): dict of n_moves (length of the row's move list;
    -1 on done and dead rows), a_star (the winning `to`, -1 without a winner), zmax (the pre-activation the target took, 0 where y = r)
    and z96 ([n, 96] pre-activations of the selecting net; omitted with z96=False).  Raises XqError when the last TD step was not a
    legal one."""
    nm, a = np.zeros(n, np.int32), np.zeros(n, np.int32)
    zm = np.zeros(n, np.float32)
    z = np.zeros((n, 96), np.float32) if z96 else None
    call("xq_dqn_last_legal", self._h, int(n), _ptr(nm, C.c_int32), _ptr(a, C.c_int32), _ptr(zm, C.c_float),
         _ptr(z, C.c_float) if z96 else None)
    out = dict(n_moves=nm, a_star=a, zmax=zm)
    if z96:
        out["z96"] = z
    return out


def _set_zero_sum(self, on=True):
    """The zero-sum (negamax) target of the batched TD step, for self-play (DESIGN.md §4 "Zero-sum target"): y = r - gamma tanh(zm)
    in place of r + gamma tanh(zm), zm as the bootstrap, td_net and precision in force leave it; n-step discounts alternate in sign;
    under set_td_bootstrap("legal") a side without a move in s' is worth -1 (y = r + gamma).  Off by default; DQN.train (the
    single-board loop) refuses it."""
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"set_zero_sum: expected a bool, got {on!r}")
    call("xq_dqn_set_zero_sum", self._h, 1 if on else 0)


def _zero_sum(self):
    """Whether the zero-sum target is in force."""
    v = C.c_int32()
    call("xq_dqn_get_zero_sum", self._h, C.byref(v))
    return bool(v.value)


DQN.set_zero_sum = _set_zero_sum
DQN.zero_sum = _zero_sum


# ---- mover view (build-defined, DESIGN.md §4 "Mover view") ----
VIEWS = {"absolute": _capi.VIEW_ABSOLUTE, "mover": _capi.VIEW_MOVER}


def _set_view(self, view="mover"):
    """ "absolute" (the default: the net reads boards as they stand) or "mover": the net reads every position from the side to move —
    view(board, side) is the board for Red and its colour swap (row -> 9 - row, Red <-> Black) for Black — and output k is the value
    of moving to square k of the view.  td_grads_replay then stages view(s, mover), the action with it and view(s', next side) from a
    ring with ReplayBuffer.track_mover() and track_next_player(); a VecEnv told set_q_view(True) picks through the same map.  The
    host and raw-pointer entry points (td_update, q_boards, getQValues, ...) take boards as the net reads them: build them with
    view_boards.  XqError while a TD step waits for its apply_grads; DQN.train refuses the mover view.  Not stored in the model
    file."""
    if view not in VIEWS:
        raise ValueError(f"set_view: expected one of {sorted(VIEWS)}, got {view!r}")
    call("xq_dqn_set_view", self._h, VIEWS[view])


def _view(self):
    """ "absolute" or "mover", as last set"""
    v = C.c_int32()
    call("xq_dqn_get_view", self._h, C.byref(v))
    return {n: k for k, n in VIEWS.items()}[v.value]


_NIBBLE_SHIFTS = (4 * np.arange(8)).astype(np.uint32)


def view_boards_packed(words, side):
    """view_boards on packed boards: [n, 12] uint32 words (square s = nibble s & 7 of word s >> 3) -> [n, 12] uint32"""
    import torch
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, _capi.BOARD_WORDS)
    n = len(w)
    s = np.ascontiguousarray(side, dtype=np.uint8).reshape(n)
    if n == 0:
        return w.copy()
    src = torch.from_numpy(w.view(np.int32)).cuda()
    sd = torch.from_numpy(s).cuda()
    out = torch.empty_like(src)
    torch.cuda.synchronize()
    call("xq_view_boards_dev", C.c_void_p(src.data_ptr()), C.c_void_p(sd.data_ptr()), n, C.c_void_p(out.data_ptr()), None)
    call("xq_stream_synchronize", None)
    return np.ascontiguousarray(out.cpu().numpy()).view(np.uint32)


def view_boards(boards, side):
    """view(board, side) of [n, 90] piece codes and [n] sides (0 = Red: the board, anything else: its colour swap) on the device
    (view_boards_kernel) -> [n, 90] uint8.  What a caller of the host entry points (td_update, getQValues, ...) feeds a net with
    set_view("mover")."""
    b = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 90)
    nib = np.zeros((len(b), 96), np.uint32)
    nib[:, :90] = b & 15
    words = (nib.reshape(-1, _capi.BOARD_WORDS, 8) << _NIBBLE_SHIFTS).sum(axis=2, dtype=np.uint32)
    out = view_boards_packed(words, side)
    return ((out[:, :, None] >> _NIBBLE_SHIFTS) & 15).reshape(-1, 96)[:, :90].astype(np.uint8)


DQN.set_view = _set_view
DQN.view = _view
DQN.set_td_bootstrap = _set_td_bootstrap
DQN.td_bootstrap = _td_bootstrap
DQN.last_legal = _last_legal


def _checked_tau(who, tau):
    tau = float(tau)
    if not 0.0 <= tau <= 1.0:
        raise ValueError(f"{who}: tau must lie in [0, 1], got {tau!r}")
    return tau


def _set_target_tau(self, tau):
    """Soft (Polyak) target update inside apply_grads / the trainer's learn_apply: theta- += tau (theta - theta-) after every update, in
    the apply kernel itself.  0 = off (default), 1 = the hard copy after every update.  After set_params / loadModel / backpropagate
    call updateTargetNetwork() once: until then a whole-buffer kernel follows every apply.  backpropagate() never moves the target."""
    call("xq_dqn_set_target_tau", self._h, _checked_tau("set_target_tau", tau))


def _target_tau(self):
    """tau in force (0.0 = off)."""
    v = C.c_double()
    call("xq_dqn_get_target_tau", self._h, C.byref(v))
    return v.value


DQN.set_target_tau = _set_target_tau
DQN.target_tau = _target_tau


def _timeline(self, max_spans=8192):
    """(name, start_ms, end_ms) of every launch bracketed in the session closed by the last kernel_stats() call."""
    arr = (KernelSpan * max_spans)()
    n = C.c_int32()
    call("xq_dqn_kernel_timeline", self._h, arr, max_spans, C.byref(n))
    return [(arr[i].name.decode(), arr[i].start_ms, arr[i].end_ms) for i in range(n.value)]


DQN.kernel_timeline = _timeline


def TrainerConfig(n_games=8192, layer_sizes=(1260, 256, 256, 8100), learning_rate=0.001, gamma=0.99, epsilon=0.1,
                  replay_capacity=1 << 20, minibatch=8192, td_net=_capi.TD_TARGET_NET,
                  backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=100, mean_gradient=1, seed=0x5EED,
                  first_game_id=0, collects_per_update=1, overlap_collect=0, prioritized=0, per_alpha=0.0, per_beta=0.0,
                  per_eps=0.0, precision=_capi.PRECISION_F32):
    c = _CConfig()
    c.n_games = n_games
    for i, s in enumerate(layer_sizes):
        c.layer_sizes[i] = int(s)
    c.n_sizes = len(layer_sizes)
    c.learning_rate, c.gamma, c.epsilon = learning_rate, gamma, epsilon
    c.replay_capacity, c.minibatch = replay_capacity, minibatch
    c.td_net, c.backprop_mode = td_net, backprop_mode
    c.target_sync_interval, c.mean_gradient = target_sync_interval, mean_gradient
    c.seed, c.first_game_id = seed, first_game_id
    c.collects_per_update = collects_per_update
    c.overlap_collect = overlap_collect
    c.prioritized, c.per_alpha, c.per_beta, c.per_eps = prioritized, per_alpha, per_beta, per_eps
    c.precision = precision
    return c


class Trainer:
    """ChessAI::train for thousands of games at once: collect() = one ply everywhere, learn_* = one minibatch update."""

    def __init__(self, config, stream=None):
        self.config = config
        h = C.c_void_p()
        call("xq_trainer_create", C.byref(config), stream, C.byref(h))
        self._h = h
        e, d, r = C.c_void_p(), C.c_void_p(), C.c_void_p()
        call("xq_trainer_env", self._h, C.byref(e))
        call("xq_trainer_dqn", self._h, C.byref(d))
        call("xq_trainer_replay", self._h, C.byref(r))
        self.env = VecEnv(0, _handle=e)
        self.dqn = DQN([config.layer_sizes[i] for i in range(config.n_sizes)], config.learning_rate, config.gamma,
                       _handle=d)
        self.replay = ReplayBuffer(0, _handle=r)

    def close(self):
        if self._h is not None:
            call("xq_trainer_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def random_plies(self, n):
        """n uniform-random plies in every game, outside the replay ring and the step counters (desynchronises the games)."""
        call("xq_trainer_random_plies", self._h, int(n))

    def set_comm(self, comm):
        call("xq_trainer_set_comm", self._h, comm.handle if comm is not None else None)

    def set_td_net(self, td_net):
        call("xq_trainer_set_td_net", self._h, int(td_net))

    def set_target_tau(self, tau):
        """DQN.set_target_tau on the trainer's network; set target_sync_interval = 0 beside it (both set: both happen).  Call between
        iterations."""
        call("xq_trainer_set_target_tau", self._h, _checked_tau("set_target_tau", tau))

    def set_n_step(self, n_step):
        """n-step TD returns from the trainer's ring (ReplayBuffer.set_n_step with stride = n_games, and the sample / hold windows that
        go with it; 1 = off).  Needs a replay ring larger than (n_step - 1 + collects_per_update) * n_games.  Call between iterations."""
        call("xq_trainer_set_n_step", self._h, int(n_step))

    def set_mirror(self, prob):
        """Mirror augmentation of every learn_grads from the trainer's ring (ReplayBuffer.set_mirror; 0 = off): each minibatch row is
        reflected left-right with probability prob.  Uniform, prioritized and on-policy, any n_step.  Call between iterations."""
        call("xq_trainer_set_mirror", self._h, float(prob))

    def set_colour_swap(self, prob):
        """Colour-swap augmentation of every learn_grads from the trainer's ring (ReplayBuffer.set_colour_swap; 0 = off): each minibatch
        row has its colours exchanged with probability prob.  Uniform, prioritized and on-policy, any n_step, self-play and versus, with
        or without the mirror.  Call between iterations."""
        call("xq_trainer_set_colour_swap", self._h, float(prob))

    def set_td_bootstrap(self, kind):
        """DQN.set_td_bootstrap on the trainer's net; "legal" first makes the trainer's ring record the side to move in s', so call it
        before the first collect (XqError once the ring holds a transition).  Back to "all" between iterations."""
        if kind not in _BOOTSTRAPS:
            raise ValueError(f"set_td_bootstrap: expected 'all' or 'legal', got {kind!r}")
        call("xq_trainer_set_td_bootstrap", self._h, _BOOTSTRAPS[kind])

    def set_view(self, view="mover"):
        """DQN.set_view on the trainer's net, VecEnv.set_q_view on its env and both side columns on its ring (DESIGN.md §4 "Mover
        view"): before the first collect (XqError afterwards).  Every collect then shows the net the boards from the side to move."""
        if view not in VIEWS:
            raise ValueError(f"set_view: expected one of {sorted(VIEWS)}, got {view!r}")
        call("xq_trainer_set_view", self._h, VIEWS[view])

    def set_zero_sum(self, on=True):
        """DQN.set_zero_sum on the trainer's net (DESIGN.md §4 "Zero-sum target"), for self-play: XqError with an opponent set, as
        set_opponent is while it is on.  Uniform, prioritized and on-policy, any n_step.  Call between iterations."""
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"set_zero_sum: expected a bool, got {on!r}")
        call("xq_trainer_set_zero_sum", self._h, 1 if on else 0)

    def set_reward(self, kind, scale=1e-3, ply_cost=0.0, bound=1.0):
        """VecEnv.set_reward on the trainer's env (DESIGN.md §4 "Reward rule"): "evaluate" (the reference's evaluateBoard, the default)
        or "delta" (the transition's change of material balance, scaled, less ply_cost, clamped to +-bound).  The next collect writes
        it; slots already in the ring keep theirs.  Call between iterations."""
        call("xq_trainer_set_reward", self._h, reward_kind(kind), float(scale), float(ply_cost), float(bound))

    def set_policy(self, kind, temperature=1.0):
        """VecEnv.set_policy on the trainer's env (DESIGN.md §4 "Exploration policy"): "greedy" (the default) or "boltzmann" at
        `temperature`.  The next collect picks by it; versus training: the learner only."""
        call("xq_trainer_set_policy", self._h, policy_kind(kind), float(temperature))

    def set_epsilon(self, eps):
        """The exploration rate of the collects from the next one queued on (TrainerConfig.epsilon), 0 <= eps <= 1; legal between any
        two collects.  Versus training: the learner's epsilon."""
        eps = float(eps)
        if not 0.0 <= eps <= 1.0:
            raise ValueError(f"set_epsilon: eps must lie in [0, 1], got {eps!r}")
        call("xq_trainer_set_epsilon", self._h, eps)

    def epsilon(self):
        v = C.c_double()
        call("xq_trainer_get_epsilon", self._h, C.byref(v))
        return v.value

    def set_opponent(self, opponent):
        """Train against a fixed opponent from the next collect on (DESIGN.md §4 "Versus training"): None = self-play (the default),
        "random" = uniform-random play, an arena.Search(depth, eps) = the material search, (DQN, eps) = a borrowed network.  The
        learner plays Black in game g iff (first_game_id + g) is odd.  Call between iterations."""
        if opponent is None:
            call("xq_trainer_set_opponent", self._h, None)
            return
        if isinstance(opponent, str) and opponent == "random":
            p = player(None)
        elif isinstance(opponent, Search):
            p = player(opponent)
        elif isinstance(opponent, tuple) and len(opponent) == 2 and isinstance(opponent[0], DQN):
            p = player(*opponent)
        else:
            raise TypeError(f"set_opponent: expected None, 'random', Search(depth, eps) or (DQN, eps), got {opponent!r}")
        call("xq_trainer_set_opponent", self._h, C.byref(p))

    def versus_results(self):
        """The learner's games against the opponent since set_opponent: wins, draws, losses, games ended and the score (W + D/2) / N."""
        out = (C.c_uint64 * 4)()
        call("xq_trainer_versus_results", self._h, out)
        w, d, l, n = (int(v) for v in out)
        return dict(wins=w, draws=d, losses=l, games=n, score=(w + 0.5 * d) / n if n else float("nan"))

    def collect(self):
        call("xq_trainer_collect", self._h)

    def learn_grads(self):
        call("xq_trainer_learn_grads", self._h)

    def learn_apply(self, world_size=1):
        call("xq_trainer_learn_apply", self._h, int(world_size))

    def step(self, n=1):
        call("xq_trainer_step", self._h, int(n))

    def synchronize(self):
        self.env.get_state(0, 1)

    def counters(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        call("xq_trainer_counters", self._h, C.byref(a), C.byref(b), C.byref(c))
        return dict(env_steps=a.value, updates=b.value, episodes=c.value)
