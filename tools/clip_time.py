"""Gradient clipping on one GPU at the headline configuration (8192 games, 1260-256-256-8100, minibatch 8192, overlapped trainer,
exact screening, layer 0 of s' derived, through the Python Trainer).

    python tools/clip_time.py [--steps 200] [--warmup 100] [--reps 3] [--clip 0.05] [--parent OTHER/libxqhip.so] [--trajectory N]

Three legs, each a fresh child process: clipping off, max_norm = +inf, a finite max_norm that clips.  Per leg one JSON line: wall ms/step
of --reps runs of --steps steps behind --warmup steps, then with the kernel statistics on the launches of every bracket and the exact
kernel time and bytes of grad_norm and sgd_apply.  --parent LIB: the off leg again on another build of the library (XQ_LIBXQHIP), in the
order other, tree, other.  --trajectory N: norm and coefficient of the first N updates from fresh weights under SGD at lr 1e-3, +inf against
the finite max_norm, and the fraction of saturated select outputs after them."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NET = (1260, 256, 256, 8100)


def trainer(xq, n, cap, seed):
    from cn_chess_ai_amd import _capi
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=0.001, gamma=0.99, epsilon=0.1, replay_capacity=cap, minibatch=n,
                           td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=10, mean_gradient=1,
                           seed=seed, first_game_id=0, overlap_collect=1, collects_per_update=1)
    t = xq.Trainer(cfg)
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    t.dqn.set_l0_derive(True)
    t.random_plies(300)
    return t


def leg(args):
    import cn_chess_ai_amd as xq
    n, cap = 8192, 1 << 18
    t = trainer(xq, n, cap, 0x5EED)
    clip = None if args.leg == "off" else float(args.leg)
    if clip is not None:
        t.dqn.set_grad_clip(clip)
    for _ in range(cap // n):
        t.collect()
    t.step(args.warmup)
    t.synchronize()
    reps = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        t.step(args.steps)
        t.synchronize()
        reps.append((time.perf_counter() - t0) * 1e3 / args.steps)
    t.dqn.kernel_stats(2)
    t.step(args.steps)
    st = {s["name"]: s for s in t.dqn.kernel_stats(0)}
    out = dict(leg=args.leg, lib=os.environ.get("XQ_LIBXQHIP", "tree"), ms_per_step=[round(x, 4) for x in reps],
               launches={k: s["launches"] for k, s in sorted(st.items())})
    for k in ("grad_norm", "sgd_apply"):
        if k in st:
            out[k + "_us"] = round(st[k]["ms"] * 1e3 / st[k]["launches"], 3)
            out[k + "_bytes"] = st[k]["bytes"] / st[k]["launches"]
    if clip is not None:
        out["stats"] = t.dqn.grad_clip_stats()
    print(json.dumps(out), flush=True)
    t.close()


def trajectory(args):
    import cn_chess_ai_amd as xq
    clip = float(args.leg)
    t = trainer(xq, 8192, 1 << 18, 0x5EED)
    t.dqn.set_grad_clip(clip)
    norms, coefs = [], []
    for _ in range(args.trajectory):
        t.step(1)
        s = t.dqn.grad_clip_stats()
        norms.append(s["last_norm"]); coefs.append(s["last_coef"])
    q = t.dqn.select_q(t.env).cpu().numpy()[:, :90]
    print(json.dumps(dict(trajectory=args.leg, norms=[float("%.4g" % x) for x in norms], coefs=[float("%.4g" % x) for x in coefs],
                          frac_select_outputs_saturated=round(float((abs(q) > 0.99).mean()), 5))), flush=True)
    t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trajectory", type=int, default=0)
    ap.add_argument("--parent")
    ap.add_argument("--clip", default="0.05")
    args = ap.parse_args()
    if args.leg:
        return trajectory(args) if args.trajectory else leg(args)
    base = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--reps", str(args.reps)]
    runs = [("off", None), ("inf", None), (args.clip, None)]
    if args.parent:
        runs += [("off", args.parent), ("off", None), ("off", args.parent)]
    for name, lib in runs:
        env = dict(os.environ)
        if lib:
            env["XQ_LIBXQHIP"] = os.path.abspath(lib)
        r = subprocess.run(base + ["--leg", name], env=env, timeout=240)
        if r.returncode != 0:
            print("leg", name, lib, "ended with", r.returncode, "- stopping", flush=True)
            return 1
    if args.trajectory:
        for name in ("inf", args.clip):
            r = subprocess.run(base + ["--leg", name, "--trajectory", str(args.trajectory)], timeout=240)
            if r.returncode != 0:
                print("trajectory", name, "ended with", r.returncode, "- stopping", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
