"""The bits and the launches of a TD step over a fixed seeded matrix, and whether another build of the library gives the same ones.

    python tools/td_step_bits.py [--forward | --rule] [--parent OTHER/libxqhip.so]

Cells: net {1260-128-8100, 1260-256-256-8100, 1260-512-512-512-8100, 1260-127-129-132-8100 (textbook rule)} x minibatch {333: one
layer-0 chunk, partial tiles; 1100: slabs everywhere, no epilogue planes; and, for the two nets of even 256 / 512 widths, 2048: whole
chunks — the planes come from the delta product's epilogue and the selector words ride in the first fused launch} x td_tail {0, 1} x
fused_apply {0, 1} x precision {fp32, BF16_FULL where the hidden widths are even} x one-rank communicator {absent, attached; skipped
when RCCL cannot be loaded}; two TD steps from one seeded self-play batch per cell.  One line per cell: a SHA-256 over the parameters,
the gradient buffer, Q(s,a), y and the (kernel name, calls) list of xq_dqn_kernel_stats.  The tests compare the paths of one build with
each other; this compares two builds — the host side of the gradient half decides which kernels run, where their partial sums go and
who adds them, and a change there that moves every path alike shows only here.
--forward: a second matrix, over what the host side of the FORWARD half decides (layer-0 form, which hidden product, where the fork
event comes from): TD rule {online, target, Double} x qmax {full, screened: fp32 net, not Double} x l0_derive {0, 1} x precision {fp32,
BF16, BF16_FULL} x the three even-width nets x minibatch {333, 1100, 2048: whole 128-row tiles and whole 256-row bf16 tiles; screening
engages from 897 samples}, hashed like the cells above; per net and batch {333, 2048} a select cell (select_q three times on the same
boards with l0_derive on: plain, kept and derived layer-0 sums; the Q rows and the kernel list); per net a trainer cell (overlapped
collect, two plies per update, 2048 games so that the select head rides on the last hidden product, screened maximum, four iterations;
the final parameters of both nets and the kernel list).  The select cells, the trainer cells and the screened / bf16 TD cells run once
more with the profiler off and without the kernel list ("prof=0"): only then does the forward product take the fork event itself.
--rule: a third matrix, over the options of the TD rule itself (xq_td.hip.h), every caller of the rule at its smallest shape: the fp32
256-wide path (1260-256-8100, 37 samples: a last block of one wave), the refine-fused step (the same net, screened maximum and fused
tail, 897 samples: the first batch at which the screen engages, its last refine block holds one sample), the fp32 512-wide path
(1260-512-8100, 37), the general path (1260-132-8100, 37), the general path with the Double fold (1260-256-8100, Double, 37) and the bf16
512-wide path with Double (1260-512-8100, BF16, 37) x loss {squared, Huber kappa 0.25} x zero_sum {0, 1} x source {the host batch, a ring
of four plies drawn prioritized, the same with n_step = 3: per_writeback_kernel}.  A combination the library refuses is printed as
refused and is no cell.  Two steps per cell; hashed: both nets' parameters, the gradient buffer, Q(s,a) and y, last_loss, the
td_error_stats record, the ring's priorities and their maximum, the kernel list.  A Huber cell prints linear/live of its last step and
counts only if 0 < linear < live, both branches of the clamp taken; otherwise the run fails.
--parent LIB: the matrix again in a fresh child process on that library (XQ_LIBXQHIP); exit status 1 if any cell differs."""
import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REF_NET = (1260, 128, 8100)
CFG2_NET = (1260, 256, 256, 8100)
CFG4_NET = (1260, 512, 512, 512, 8100)
SCALAR_NET = (1260, 127, 129, 132, 8100)
SHAPES = [(REF_NET, (333, 1100)), (CFG2_NET, (333, 1100, 2048)), (CFG4_NET, (333, 1100, 2048)), (SCALAR_NET, (333, 1100))]


def selfplay_batch(xq, n, seed):
    import numpy as np
    env = xq.VecEnv(n, seed=seed)
    for _ in range(13):
        env.selfplay_step(None)
    S, _ = env.get_state()
    res = env.selfplay_step(None)
    S2, _ = env.get_state()
    env.close()
    D = res["done"].copy()
    D[::7] = 1
    return S, S2, (res["action"] % 90).astype(np.int32), (res["reward"] / 100.0).astype(np.float32), D


def seeded_net(xq, sizes, precision):
    import numpy as np
    d = xq.DQN(sizes, 0.001, 0.99, seed=5)
    rng = np.random.default_rng(len(sizes) * 1000 + sizes[1])
    d.set_params(rng.uniform(-0.05, 0.05, size=d.n_weights), rng.uniform(-0.05, 0.05, size=d.n_biases))
    d.updateTargetNetwork()
    d.set_precision(precision)
    return d


def cell(xq, sizes, batch, n, tail, fused, precision, comm):
    import numpy as np
    import torch
    from cn_chess_ai_amd import _capi, dist as xd
    d = seeded_net(xq, sizes, precision)
    d.set_td_tail(tail)
    d.set_fused_apply(fused)
    if comm is not None:
        d.set_comm(comm)
    # the reference's backward rule is undefined where a hidden layer widens (127 -> 129 -> 132): the textbook rule there
    mode = _capi.BACKPROP_TEXTBOOK if sizes == SCALAR_NET else _capi.BACKPROP_REFERENCE
    h = hashlib.sha256()
    d.kernel_stats(enable=2)
    for _ in range(2):
        qsa, y = d.td_update(*batch, td_net=0, mode=mode, learning_rate=0.05, grad_scale=1.0 / n)
        h.update(qsa.tobytes()); h.update(y.tobytes())
    launches = sorted((k["name"], k["launches"]) for k in d.kernel_stats(enable=0))
    h.update(json.dumps(launches).encode())
    for x in d.get_params():
        h.update(np.ascontiguousarray(x).tobytes())
    ptr, k = d.grad_buffer()
    torch.cuda.synchronize()
    h.update(xd.wrap_device_floats(ptr, k).cpu().numpy().tobytes())
    d.close()
    return h.hexdigest()


def matrix():
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi, dist as xd
    out, skipped = {}, []
    try:
        comm = xd.Comm(rank=0, world=1)
    except Exception as e:                         # no RCCL on this machine: the cells with a communicator are skipped, and counted
        comm = None
        print("no communicator:", e, flush=True)
    for sizes, ns in SHAPES:
        for n in ns:
            batch = selfplay_batch(xq, n, seed=83)
            for tail, fused, prec, with_comm in itertools.product((0, 1), (0, 1), (_capi.PRECISION_F32, _capi.PRECISION_BF16_FULL), (0, 1)):
                if prec and any(x & 1 for x in sizes[1:-1]):
                    continue                       # (the bf16 Q-net needs even hidden widths: not a cell)
                name = "%s n=%d tail=%d fused=%d %s comm=%d" % ("-".join(map(str, sizes)), n, tail, fused, "bf16_full" if prec else "fp32", with_comm)
                if with_comm and comm is None:
                    skipped.append(name)
                    continue
                out[name] = cell(xq, sizes, batch, n, tail, fused, prec, comm if with_comm else None)
                print(out[name], name, flush=True)
    if comm is not None:
        comm.close()
    print("%d cells run, %d skipped (no communicator)" % (len(out), len(skipped)), flush=True)
    return out


def kernel_list(d, h, prof):
    """The (name, calls) list into the hash, and the profiler off again (prof = 0: it never was on, nothing is hashed)."""
    if prof:
        h.update(json.dumps(sorted((k["name"], k["launches"]) for k in d.kernel_stats(enable=0))).encode())


def forward_td_cell(xq, sizes, batch, n, td_net, screened, derive, precision, prof):
    import numpy as np
    import torch
    from cn_chess_ai_amd import _capi, dist as xd
    d = seeded_net(xq, sizes, precision)
    rng = np.random.default_rng(sizes[1] + 7)                  # a target net of its own: the target and Double rules read other weights
    d.set_params(rng.uniform(-0.05, 0.05, size=d.n_weights), rng.uniform(-0.05, 0.05, size=d.n_biases), net=_capi.NET_TARGET)
    d.set_qmax_mode(_capi.QMAX_SCREENED if screened else _capi.QMAX_FULL)
    d.set_l0_derive(derive)
    h = hashlib.sha256()
    if prof:
        d.kernel_stats(enable=2)
    for _ in range(2):
        qsa, y = d.td_update(*batch, td_net=td_net, mode=_capi.BACKPROP_REFERENCE, learning_rate=0.05, grad_scale=1.0 / n)
        h.update(qsa.tobytes()); h.update(y.tobytes())
    kernel_list(d, h, prof)
    for x in d.get_params():
        h.update(np.ascontiguousarray(x).tobytes())
    ptr, k = d.grad_buffer()
    torch.cuda.synchronize()
    h.update(xd.wrap_device_floats(ptr, k).cpu().numpy().tobytes())
    d.close()
    return h.hexdigest()


def select_cell(xq, sizes, n, prof):
    from cn_chess_ai_amd import _capi
    env = xq.VecEnv(n, seed=29)
    for _ in range(13):
        env.selfplay_step(None)
    d = seeded_net(xq, sizes, _capi.PRECISION_F32)
    d.set_l0_derive(True)
    h = hashlib.sha256()
    if prof:
        d.kernel_stats(enable=2)
    for _ in range(3):                                 # the first call of a period keeps nothing, the second keeps, the third derives
        h.update(d.select_q(env).cpu().numpy().tobytes())
    kernel_list(d, h, prof)
    env.close(); d.close()
    return h.hexdigest()


def trainer_cell(xq, sizes, prof):
    import numpy as np
    from cn_chess_ai_amd import _capi
    cfg = xq.TrainerConfig(n_games=2048, layer_sizes=sizes, replay_capacity=1 << 14, minibatch=2048, collects_per_update=2,
                           target_sync_interval=2, td_net=_capi.TD_ONLINE_NET, overlap_collect=1, seed=0x5EED, first_game_id=2048)
    t = xq.Trainer(cfg)
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    t.dqn.set_l0_derive(True)
    t.random_plies(20)
    h = hashlib.sha256()
    if prof:
        t.dqn.kernel_stats(enable=2)
    t.step(4)
    t.synchronize()
    kernel_list(t.dqn, h, prof)
    for net in (_capi.NET_ONLINE, _capi.NET_TARGET):
        for x in t.dqn.get_params(net=net):
            h.update(np.ascontiguousarray(x).tobytes())
    t.close()
    return h.hexdigest()


def forward_matrix():
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    out = {}

    def run(name, f, *a):
        out[name] = f(xq, *a)
        print(out[name], name, flush=True)

    precisions = ((_capi.PRECISION_F32, "fp32"), (_capi.PRECISION_BF16, "bf16"), (_capi.PRECISION_BF16_FULL, "bf16_full"))
    for sizes in (REF_NET, CFG2_NET, CFG4_NET):
        net = "-".join(map(str, sizes))
        for n in (333, 1100, 2048):
            batch = selfplay_batch(xq, n, seed=83)
            for td_net, screened, derive, (prec, pname) in itertools.product((0, 1, 2), (0, 1), (0, 1), precisions):
                if screened and (prec != _capi.PRECISION_F32 or td_net == _capi.TD_DOUBLE):
                    continue                       # (the screened maximum is defined for the fp32 net and one s' chain: not a cell)
                for prof in ((1, 0) if screened or prec != _capi.PRECISION_F32 else (1,)):
                    run("td %s n=%d rule=%d screened=%d derive=%d %s prof=%d" % (net, n, td_net, screened, derive, pname, prof),
                        forward_td_cell, sizes, batch, n, td_net, screened, derive, prec, prof)
        for n, prof in itertools.product((333, 2048), (1, 0)):
            run("select %s n=%d prof=%d" % (net, n, prof), select_cell, sizes, n, prof)
        for prof in (1, 0):
            run("trainer %s prof=%d" % (net, prof), trainer_cell, sizes, prof)
    print("%d cells run" % len(out), flush=True)
    return out


RULE_CALLERS = [   # name, net, batch, TD rule, precision (a _capi name), screened maximum + fused tail
    ("f32_256", (1260, 256, 8100), 37, 0, "PRECISION_F32", False),
    ("refine_fused", (1260, 256, 8100), 897, 0, "PRECISION_F32", True),
    ("f32_512", (1260, 512, 8100), 37, 0, "PRECISION_F32", False),
    ("general", (1260, 132, 8100), 37, 0, "PRECISION_F32", False),
    ("general_double", (1260, 256, 8100), 37, 2, "PRECISION_F32", False),
    ("bf16_512_double", (1260, 512, 8100), 37, 2, "PRECISION_BF16", False),
]
RULE_KAPPA = 0.25
RULE_PLIES = 4                     # the ring: four consecutive plies of n games, so that a chain of three is a real one


def ring_plies(xq, n, seed):
    """RULE_PLIES consecutive self-play plies of n games as (S, A, R, D, S2) per ply, every seventh row of a ply terminal"""
    import numpy as np
    env = xq.VecEnv(n, seed=seed)
    for _ in range(13):
        env.selfplay_step(None)
    plies = []
    for _ in range(RULE_PLIES):
        S, _ = env.get_state()
        res = env.selfplay_step(None)
        S2, _ = env.get_state()
        D = res["done"].copy()
        D[::7] = 1
        plies.append((S, (res["action"] % 90).astype(np.int32), (res["reward"] / 100.0).astype(np.float32), D, S2))
    env.close()
    return plies


def rule_cell(xq, sizes, n, td_net, precision, screened, huber, zero_sum, source, plies):
    import numpy as np
    import torch
    from cn_chess_ai_amd import _capi, dist as xd
    d = seeded_net(xq, sizes, precision)
    rng = np.random.default_rng(sizes[1] + 7)                  # a target net of its own: the Double rule reads other weights
    d.set_params(rng.uniform(-0.05, 0.05, size=d.n_weights), rng.uniform(-0.05, 0.05, size=d.n_biases), net=_capi.NET_TARGET)
    rp = None
    try:
        d.set_qmax_mode(_capi.QMAX_SCREENED if screened else _capi.QMAX_FULL)
        d.set_td_tail(screened)
        if huber:
            d.set_td_loss("huber", RULE_KAPPA)
        d.set_zero_sum(bool(zero_sum))
        if source != "host":
            rp = xq.ReplayBuffer(RULE_PLIES * n, seed=0xFEED + n)
            rp.enable_per(0.6, 0.4, 1e-3)
            for p in plies:
                rp.push(*p)
            rp.set_priorities(np.random.default_rng(7).uniform(0.05, 2.0, size=RULE_PLIES * n).astype(np.float32))
            if source == "per_n3":
                rp.set_n_step(3, n)
        h = hashlib.sha256()
        d.kernel_stats(enable=2)
        for _ in range(2):
            if rp is None:
                S, A, R, D, S2 = plies[0]
                d.td_update(S, S2, A, R, D, td_net=td_net, mode=_capi.BACKPROP_REFERENCE, learning_rate=0.05, grad_scale=1.0 / n)
            else:
                rp.per_rebuild()
                rp.sample_prioritized(n, host=False)
                d.td_grads_replay(rp, n, td_net=td_net, mode=_capi.BACKPROP_REFERENCE)
                d.apply_grads(0.05, 1.0 / n)
            for x in d.last_td_values(n):
                h.update(x.tobytes())
            st = d.td_error_stats()
            h.update(json.dumps([d.last_loss()] + [st[k] for k in ("live", "mean_abs", "max_abs", "mean_loss", "linear")]).encode())
        kernel_list(d, h, 1)
        for net in (_capi.NET_ONLINE, _capi.NET_TARGET):
            for x in d.get_params(net=net):
                h.update(np.ascontiguousarray(x).tobytes())
        ptr, k = d.grad_buffer()
        torch.cuda.synchronize()
        h.update(xd.wrap_device_floats(ptr, k).cpu().numpy().tobytes())
        if rp is not None:
            rp.per_rebuild()
            h.update(rp.get_priorities(0, RULE_PLIES * n).tobytes())
            h.update(json.dumps(rp.per_stats()["max_priority"]).encode())
        return h.hexdigest(), st["linear"], st["live"]
    finally:
        d.close()
        if rp is not None:
            rp.close()


def rule_matrix():
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    out, refused, one_sided = {}, 0, []
    rings = {}
    for (cname, sizes, n, td_net, prec, screened), huber, zero_sum, source in itertools.product(RULE_CALLERS, (0, 1), (0, 1), ("host", "per", "per_n3")):
        if n not in rings:
            rings[n] = ring_plies(xq, n, seed=83)
        name = "rule %s %s n=%d loss=%s zero_sum=%d source=%s" % (cname, "-".join(map(str, sizes)), n, "huber" if huber else "squared", zero_sum, source)
        try:
            digest, linear, live = rule_cell(xq, sizes, n, td_net, getattr(_capi, prec), screened, huber, zero_sum, source, rings[n])
        except xq.XqError as e:
            refused += 1
            print("refused", name, "--", str(e).splitlines()[0], flush=True)
            continue
        out[name] = digest
        print(digest, name, ("linear/live %d/%d" % (linear, live)) if huber else "", flush=True)
        if huber and not 0 < linear < live:
            one_sided.append(name)
    for name in one_sided:
        print("ONE-SIDED CLAMP", name, flush=True)
    print("%d cells run, %d refused, %d Huber cells with a one-sided clamp" % (len(out), refused, len(one_sided)), flush=True)
    if one_sided:
        sys.exit(2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--forward", action="store_true", help="the forward-half matrix instead of the gradient-half one")
    ap.add_argument("--rule", action="store_true", help="the matrix over the TD rule's options and callers instead")
    ap.add_argument("--json", action="store_true", help="(the child process of --parent) the cells as one JSON line at the end")
    args = ap.parse_args()
    which = ["--forward"] if args.forward else ["--rule"] if args.rule else []
    mine = forward_matrix() if args.forward else rule_matrix() if args.rule else matrix()
    if args.json:
        print("CELLS " + json.dumps(mine), flush=True)
    if not args.parent:
        return 0
    env = dict(os.environ, XQ_LIBXQHIP=os.path.abspath(args.parent))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--json"] + which, env=env,
                       stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        print("the run on", args.parent, "ended with", r.returncode, flush=True)
        return 1
    other = json.loads([l for l in r.stdout.splitlines() if l.startswith("CELLS ")][-1][6:])
    differ = [k for k in mine if other.get(k) != mine[k]]
    for k in differ:
        print("DIFFERS", k, mine[k], other.get(k), flush=True)
    print("%d cells, %d differ" % (len(mine), len(differ)), flush=True)
    return 1 if differ or len(other) != len(mine) else 0


if __name__ == "__main__":
    sys.exit(main())
