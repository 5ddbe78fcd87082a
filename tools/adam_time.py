"""The Adam apply against the SGD apply on one GPU, and what each optimizer does to the select outputs in a sustained run.

    python tools/adam_time.py [--steps 200] [--warmup 50] [--saturation N] [--pairs 2048]

Timing: the headline configuration (8192 games, 1260-256-256-8100, 1 M ring filled to capacity, overlapped collect, exact screening,
layer 0 of s' derived, fused launches, slab sums inside the optimizer kernel), both optimizers in ONE process: --warmup steps, then
--steps steps with the kernel statistics on; `sgd_apply` / `adam_apply` are exact kernel times (the launches carry their own start and
stop events), ms/step is wall time of the same steps with the statistics off.  byte_ratio is workmodel's.
--saturation N: N updates under each optimizer from the same seed (lr 1e-3, Adam's defaults), then the fraction of the select outputs
Q(s)[0..89] of the trainer's boards with |Q| > 0.99 and the net's arena score against random play.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import cn_chess_ai_amd as xq                       # noqa: E402
from cn_chess_ai_amd import _capi, workmodel      # noqa: E402

NET = (1260, 256, 256, 8100)


def trainer(n, cap, seed, opt):
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=0.001, gamma=0.99, epsilon=0.1, replay_capacity=cap, minibatch=n,
                           td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=10, mean_gradient=1,
                           seed=seed, first_game_id=0, overlap_collect=1, collects_per_update=1)
    t = xq.Trainer(cfg)
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    t.dqn.set_l0_derive(True)
    t.dqn.set_optimizer(opt)
    t.random_plies(300)
    return t


def timing(args):
    n, cap = args.games, 1 << 20
    out = {}
    for opt in ("sgd", "adam"):
        t = trainer(n, cap, 0x5EED, opt)
        for _ in range(cap // n):
            t.collect()
        t.step(args.warmup)
        t.synchronize()
        t0 = time.perf_counter()
        t.step(args.steps)
        t.synchronize()
        ms_step = (time.perf_counter() - t0) * 1e3 / args.steps
        t.dqn.kernel_stats(2)
        t.step(args.steps)
        st = {s["name"]: s for s in t.dqn.kernel_stats(0)}
        k = st[opt + "_apply"]
        assert k["exact"] == k["launches"] == args.steps and ("adam_apply" in st) == (opt == "adam")
        out[opt] = dict(us=k["ms"] * 1e3 / k["launches"], ms_step=ms_step)
        t.close()
    w = {o: workmodel.step_work(NET, n, n, optimizer=o)[o + "_apply"]["hbm_bytes"] for o in ("sgd", "adam")}
    print(json.dumps(dict(measure="apply_kernel_us", games=n, steps=args.steps, warmup=args.warmup, sgd_apply_us=round(out["sgd"]["us"], 3),
                          adam_apply_us=round(out["adam"]["us"], 3), ratio=round(out["adam"]["us"] / out["sgd"]["us"], 4),
                          byte_ratio=round(w["adam"] / w["sgd"], 4), sgd_ms_per_step=round(out["sgd"]["ms_step"], 4),
                          adam_ms_per_step=round(out["adam"]["ms_step"], 4))), flush=True)


def saturation(args):
    n = args.games
    for opt in ("sgd", "adam"):
        t = trainer(n, 1 << 20, 0x5EED, opt)
        t.set_opponent("random")
        t.step(args.saturation)
        t.synchronize()
        q = t.dqn.select_q(t.env).cpu().numpy()[:, :90]
        vs = t.versus_results()
        a = xq.Arena(args.pairs, seed=77)
        a.run(t.dqn, None, 0.0, 0.0)
        s = a.summary()
        print(json.dumps(dict(measure="saturation", optimizer=opt, updates=args.saturation, lr=0.001,
                              frac_select_outputs_saturated=round(float((abs(q) > 0.99).mean()), 5), versus_results=vs,
                              arena_vs_random=dict(score=round(s["score"], 4), wins=s["wins"], draws=s["draws"], losses=s["losses"]))),
              flush=True)
        a.close(); t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--saturation", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--no-timing", action="store_true")
    args = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("no HIP device")
    if not args.no_timing:
        timing(args)
    if args.saturation > 0:
        saturation(args)


if __name__ == "__main__":
    main()
