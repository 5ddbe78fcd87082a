"""Kernel time of a TD step from a ring with n-step returns off and on, at 8192 x 1260-256-256-8100 from a ring of 1 M transitions, from
the handle's own kernel-exact events (xq_dqn_kernel_stats): n_step = 1 and n_step = 3, each leg twice and alternating, in one command.
The ring is filled by self-play of 8192 games (stride 8192), so the chains are real trajectories.  Reports, per leg, the microseconds
per launch of nstep_assemble and the sum over every bracketed kernel of the step (the layer-0 derivation of s' from s spans up to 2n
changed squares with n-step next boards).  Prints one JSON object; profiles/NOTES.md ("n-step returns") says what to set it against.

    python tools/nstep_time.py [--steps 40] [--ring 1048576]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--ring", type=int, default=1 << 20)
    ap.add_argument("--n-step", type=int, default=3)
    args = ap.parse_args()
    import torch
    import cn_chess_ai_amd as xq
    from test_dqn_gpu import CFG2_NET, make_net
    n = 8192
    env = xq.VecEnv(n, seed=77)
    rp = xq.ReplayBuffer(args.ring, seed=1)
    d, _, _ = make_net(xq, CFG2_NET, seed=5)
    d.set_fused_apply(True)
    d.set_qmax_mode(xq._capi.QMAX_SCREENED)
    d.set_l0_derive(True)
    for _ in range((args.ring + n - 1) // n):                    # fill the ring: one collect = 8192 slots
        q = d.q_boards(env, 96)
        env.selfplay_step_dev(q.data_ptr(), 96, 0.3, replay=rp)
    torch.cuda.synchronize()
    assert rp.stats()[0] == args.ring
    out = {}
    for leg, ns in (("n1", 1), ("n%d" % args.n_step, args.n_step), ("n1_again", 1), ("n%d_again" % args.n_step, args.n_step)):
        rp.set_n_step(ns, n)
        for _ in range(2):                                       # the first round warms up
            d.kernel_stats(2)
            for _ in range(args.steps):
                rp.sample(n, host=False)
                d.td_grads_replay(rp, n, td_net=0, mode=0)
                d.apply_grads(1e-3, 1.0 / n)
            st = {s["name"]: s for s in d.kernel_stats(0)}
        r = dict(step_kernel_sum_us=1e3 * sum(s["ms"] for s in st.values()) / args.steps,
                 kernels={k: round(1e3 * s["ms"] / s["launches"], 2) for k, s in st.items()})
        if "nstep_assemble" in st:
            a = st["nstep_assemble"]
            r["nstep_assemble_us"] = 1e3 * a["ms"] / a["launches"]
            r["exact"], r["launches"] = a["exact"], a["launches"]
            ls = d.last_n_step(n)
            r["dead_rows"] = int((ls["action"] < 0).sum())
            r["mean_steps"] = float(ls["steps"].mean())
        out[leg] = r
    print(json.dumps(out))
    rp.close(); d.close(); env.close()


if __name__ == "__main__":
    main()
