"""The bits of xq_dqn_apply_grads over a fixed seeded matrix, and whether another build of the library gives the same ones.

    python tools/apply_bits.py [--parent OTHER/libxqhip.so]

Cells: net {1260-128-8100, 1260-256-256-8100, 1260-127-129-132-8100 (segments off 16 bytes and of odd length: the scalar loops)} x optimizer
{sgd, adam} x clip {off, +inf, a max_norm that clips} x fused_apply {0, 1} x precision {fp32, bf16 with its shadow; the bf16 Q-net
needs even hidden widths, so 1260-127-129-132-8100 runs in fp32 only} x minibatch {1300, and 8192 for 1260-256-256-8100}; three TD steps
from one seeded ring per cell.  One line per cell: a SHA-256 over the parameters, Adam's m and v, the gradient buffer and the clip
record.  The tests compare the paths of one build with each other; this compares two builds, which is what catches a change that moves
every path alike (another contraction of an element update, say).
--parent LIB: the matrix again in a fresh child process on that library (XQ_LIBXQHIP); exit status 1 if any cell differs."""
import argparse
import hashlib
import itertools
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REF_NET = (1260, 128, 8100)
CFG2_NET = (1260, 256, 256, 8100)
SCALAR_NET = (1260, 127, 129, 132, 8100)
CLIP = 1e-3                                        # below every norm these steps see (checked)


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
    return S, (res["action"] % 90).astype(np.int32), (res["reward"] / 100.0).astype(np.float32), D, S2


def cell(xq, sizes, batch, n, opt, clip, fused, precision):
    import numpy as np
    import torch
    from cn_chess_ai_amd import _capi, dist as xd
    d = xq.DQN(sizes, 0.001, 0.99, seed=5)
    rng = np.random.default_rng(len(sizes) * 1000 + sizes[1])
    d.set_params(rng.uniform(-0.05, 0.05, size=d.n_weights), rng.uniform(-0.05, 0.05, size=d.n_biases))
    d.updateTargetNetwork()
    d.set_precision(precision)
    d.set_optimizer(opt)
    d.set_fused_apply(fused)
    d.set_grad_clip(clip)
    rp = xq.ReplayBuffer(n, seed=0xABC)
    rp.push(*batch)
    # the reference's backward rule is undefined where a hidden layer widens (127 -> 129 -> 132): the textbook rule there
    mode = _capi.BACKPROP_TEXTBOOK if sizes == SCALAR_NET else _capi.BACKPROP_REFERENCE
    h = hashlib.sha256()
    clipped = 0
    for _ in range(3):
        rp.sample(n)
        d.td_grads_replay(rp, n, td_net=0, mode=mode)
        d.apply_grads(1e-2, 1.0 / n)
        if clip:
            st = d.grad_clip_stats()
            clipped = st["clipped"]
            h.update(json.dumps(st, sort_keys=True).encode())
    for x in d.get_params():
        h.update(np.ascontiguousarray(x).tobytes())
    if opt == "adam":
        m, v, t = d.optimizer_state()
        h.update(m.tobytes()); h.update(v.tobytes()); h.update(str(t).encode())
    ptr, k = d.grad_buffer()
    torch.cuda.synchronize()
    h.update(xd.wrap_device_floats(ptr, k).cpu().numpy().tobytes())
    rp.close(); d.close()
    if (clipped >= 1) != (clip == CLIP):
        raise SystemExit("max_norm %g clipped %d of 3 steps of %s" % (clip, clipped, sizes))
    return h.hexdigest()


def matrix():
    import cn_chess_ai_amd as xq
    from cn_chess_ai_amd import _capi
    out = {}
    for sizes, n in [(REF_NET, 1300), (CFG2_NET, 1300), (SCALAR_NET, 1300), (CFG2_NET, 8192)]:
        batch = selfplay_batch(xq, n, seed=83)
        for opt, clip, fused, prec in itertools.product(("sgd", "adam"), (0.0, math.inf, CLIP), (0, 1),
                                                        (_capi.PRECISION_F32, _capi.PRECISION_BF16)):
            if prec and any(x & 1 for x in sizes[1:-1]):
                continue
            name = "%s n=%d %s clip=%g fused=%d %s" % ("-".join(map(str, sizes)), n, opt, clip, fused, "bf16" if prec else "fp32")
            out[name] = cell(xq, sizes, batch, n, opt, clip, fused, prec)
            print(out[name], name, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--json", action="store_true", help="(the child process of --parent) the cells as one JSON line at the end")
    args = ap.parse_args()
    mine = matrix()
    if args.json:
        print("CELLS " + json.dumps(mine), flush=True)
    if not args.parent:
        return 0
    env = dict(os.environ, XQ_LIBXQHIP=os.path.abspath(args.parent))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--json"], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
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
