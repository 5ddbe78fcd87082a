"""Does self-play learn better when the net reads every position from the side to move?  tools/zero_sum_curve.py's recipe with the
zero-sum target on, trained twice — absolute view, mover view — and scored in the arena as training goes on.

    python tools/view_curve.py [--games 4096] [--iters 4000] [--every 500] [--pairs 2048] [--out profiles/view_curve.json]

The recipe is tools/learn_curve.py's with the opponent taken away: SELF-PLAY, 1260-256-256-8100, ring of 64 collects, overlapped collect,
epsilon 0.1, Adam (lr 1e-4), Huber loss (kappa 1), legal-move bootstrap, the target-network rule on a soft target (tau 0.01), gradient
clipped at norm 10, reward delta(1e-3, 0, 1), the zero-sum target (Trainer.set_zero_sum).  Trained once with the absolute view and once
with the mover view (Trainer.set_view("mover"): collects, ring step and the arena read Black's positions colour-swapped), from the same
seeds.  Every --every iterations (and before the first) the greedy net plays --pairs pairs of arena games against uniform-random play
and against the depth-1 material search; the scores with their 95 % intervals go to --out as JSON, one line per checkpoint to stdout.
A recorded result, not a gate, and one seed shows a direction only: profiles/NOTES.md ("Mover view") says what came out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NET = (1260, 256, 256, 8100)
REWARD = ("delta", 1e-3, 0.0, 1.0)


def score(xq, dqn, opponent, pairs):
    a = xq.Arena(pairs, seed=77)
    a.run(dqn, opponent, 0.0, 0.0)
    s = a.summary()
    a.close()
    return dict(score=round(s["score"], 4), ci95=[round(x, 4) for x in s["ci95"]], wins=s["wins"], draws=s["draws"], losses=s["losses"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--every", type=int, default=500)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_curve.json"))
    args = ap.parse_args()
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    n = args.games
    recipe = dict(games=n, net=list(NET), ring=64 * n, minibatch=n, epsilon=0.1, optimizer="adam", lr=args.lr, loss="huber(1)",
                  bootstrap="legal", td_net="target", target_tau=0.01, grad_clip=10.0, gamma=0.99, opponent=None, reward=list(REWARD), zero_sum=True,
                  seed=0x5EED, arena_pairs=args.pairs, arena_opening_plies=8,
                  arena="greedy net against uniform-random play and against Search(1)")
    legs = []
    for view in ("absolute", "mover"):
        cfg = xq.TrainerConfig(n_games=n, layer_sizes=NET, learning_rate=args.lr, gamma=0.99, epsilon=0.1, replay_capacity=64 * n,
                               minibatch=n, td_net=_capi.TD_TARGET_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=0,
                               mean_gradient=1, seed=0x5EED, first_game_id=0, overlap_collect=1, collects_per_update=1)
        t = xq.Trainer(cfg)
        t.set_td_bootstrap("legal")                  # (before the first collect: the ring records the side to move in s')
        t.dqn.set_optimizer("adam")
        t.dqn.set_td_loss("huber", 1.0)
        t.dqn.set_grad_clip(10.0)
        t.set_target_tau(0.01)
        t.set_reward(*REWARD)
        t.set_zero_sum(True)
        t.set_view(view)                             # (before the first collect too: the ring records who moved)
        curve, done, train_s = [], 0, 0.0
        while True:
            t.synchronize()
            td = t.dqn.td_error_stats() if done else None           # (of the last TD step, before the arena borrows the net)
            point = dict(view=view, iterations=done, train_seconds=round(train_s, 2),
                         vs_random=score(xq, t.dqn, None, args.pairs), vs_search1=score(xq, t.dqn, xq.Search(1, 0.0), args.pairs))
            point["td_error"] = td
            curve.append(point)
            print(json.dumps(point), flush=True)
            if done >= args.iters:
                break
            k = min(args.every, args.iters - done)
            t0 = time.perf_counter()
            t.step(k)
            t.synchronize()
            train_s += time.perf_counter() - t0
            done += k
        legs.append(dict(view=view, curve=curve))
        t.close()
    with open(args.out, "w") as f:
        json.dump(dict(recipe=recipe, legs=legs), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
