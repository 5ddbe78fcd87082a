"""Versus training on one GPU: the cost of a collect against each opponent, and a small strength run.

    python tools/versus_time.py [--games 8192] [--collects 50] [--strength N] [--pairs 4096]

Timing: ms per trainer collect at --games games (1260-256-256-8100 learner, sequential trainer), self-play against random play,
search-1, search-2 and a borrowed network of the same shape; wall time of --collects collects after 5 warm-up collects, the stream
synchronised before and after.  --strength N: the same net trained N updates against search-1 and N updates by self-play from the
same seed (bench composition: 1 M ring, overlapped collect, screened max), then each scored with the Arena against Search(1) and
against random play at --pairs pairs.  One JSON line per measurement.
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
from cn_chess_ai_amd import _capi                 # noqa: E402

NET = (1260, 256, 256, 8100)


def trainer(n, cap, minibatch, seed, overlap=0):
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=0.001, gamma=0.99, epsilon=0.1, replay_capacity=cap,
                           minibatch=minibatch, td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE,
                           target_sync_interval=10, mean_gradient=1, seed=seed, first_game_id=0, overlap_collect=overlap,
                           collects_per_update=1)
    return xq.Trainer(cfg)


def time_collects(args):
    opp_net = xq.DQN(NET, 0.001, 0.99, seed=3)
    for name, opp in [("selfplay", None), ("random", "random"), ("search1", xq.Search(1)), ("search2", xq.Search(2)),
                      ("net", (opp_net, 0.0))]:
        t = trainer(args.games, 4 * args.games, args.games, 11)
        t.random_plies(40)
        t.set_opponent(opp)
        for _ in range(5):
            t.collect()
        t.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.collects):
            t.collect()
        t.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.collects
        line = dict(measure="collect_ms", opponent=name, games=args.games, collects=args.collects, ms_per_collect=round(ms, 4))
        if opp is not None:
            line["versus"] = t.versus_results()
        print(json.dumps(line), flush=True)
        t.close()
    opp_net.close()


def strength(args):
    seed = 0x5EED
    scores = {}
    for name, opp in [("search1", xq.Search(1)), ("selfplay", None)]:
        t = trainer(args.games, 1 << 20, args.games, seed, overlap=1)
        t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
        t.random_plies(300)
        t.set_opponent(opp)
        t0 = time.perf_counter()
        t.step(args.strength)
        t.synchronize()
        secs = time.perf_counter() - t0
        vs = t.versus_results() if opp is not None else None
        for foe_name, foe in [("search1", xq.Search(1)), ("random", None)]:
            a = xq.Arena(args.pairs, seed=77)
            a.run(t.dqn, foe, 0.0, 0.0)
            s = a.summary()
            scores[(name, foe_name)] = s
            print(json.dumps(dict(measure="strength", trained=name, updates=args.strength, train_s=round(secs, 2), against=foe_name,
                                  pairs=args.pairs, score=round(s["score"], 4), ci95=[round(x, 4) for x in s["ci95"]],
                                  wins=s["wins"], draws=s["draws"], losses=s["losses"], training_versus=vs)), flush=True)
            a.close()
        t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=8192)
    ap.add_argument("--collects", type=int, default=50)
    ap.add_argument("--strength", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--no-timing", action="store_true")
    args = ap.parse_args()
    if _capi.device_count() < 1:
        raise SystemExit("no HIP device")
    if not args.no_timing:
        time_collects(args)
    if args.strength > 0:
        strength(args)


if __name__ == "__main__":
    main()
