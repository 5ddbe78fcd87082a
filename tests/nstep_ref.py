"""Reference of the n-step TD returns (include/xq_capi.h, xq_replay_set_n_step; DESIGN.md §4 "n-step returns"): a plain per-row loop in
np.float32 over the ring's arrays, an independent per-trajectory walk in fp64 over the push order, seeded fixtures, and three deliberately
wrong references (negative controls).  No device, no library: the GPU tests compare the library with assemble()."""
import numpy as np

CLASSES_FIXED = ("full", "incomplete", "empty0", "empty_mid")


def classes(n):
    """every class of row an n-step batch can hold"""
    return CLASSES_FIXED + tuple(f"done{m}" for m in range(1, n + 1))


def discounts(gamma, n):
    """disc_0 = 1, disc_k = fl32(disc_{k-1} * (float)gamma), k = 0..n"""
    gf = np.float32(gamma)
    d = [np.float32(1.0)]
    for _ in range(n):
        d.append(np.float32(d[-1] * gf))
    return d


def readable(cap, size, write_pos):
    """the default readable range: `size` slots in age order from slot 0 (ring not full) or from the write position (full)"""
    return (0 if size < cap else write_pos), size


def assemble(A, R, D, cap, slots, n, stride, gamma, first, count, wrong=None):
    """The definition, row by row.  A, R, D: action_to / reward / done by ring slot.  wrong: None, or one of the negative controls
    "ignore_done" (never stops at done), "plus_one" (walks +1 instead of +stride), "incomplete_live" (a chain that leaves the readable
    range is cut short and stays live)."""
    disc = discounts(gamma, n)
    step = 1 if wrong == "plus_one" else stride
    out = dict(reward=[], done=[], steps=[], first_slot=[], last_slot=[], action=[], dead=[], cls=[])
    for s in slots:
        s = int(s)
        off0 = (s - first) % cap
        Rn, Dn, m, last = np.float32(R[s]), bool(D[s]), 1, s
        dead = A[s] < 0
        cls = "empty0" if dead else None
        if not dead:
            for k in range(1, n):
                if Dn and wrong != "ignore_done":
                    break
                off = off0 + k * step
                slot = (first + off) % cap
                if not off < count:
                    if wrong == "incomplete_live":
                        break
                    dead, cls = True, "incomplete"
                    break
                if A[slot] < 0:
                    dead, cls = True, "empty_mid"
                    break
                Rn = np.float32(Rn + np.float32(disc[k] * np.float32(R[slot])))
                Dn, m, last = bool(D[slot]), k + 1, slot
        if cls is None:
            cls = f"done{m}" if Dn else ("full" if m == n else "cut")
        out["reward"].append(Rn); out["done"].append(1 if Dn else 0); out["steps"].append(m)
        out["first_slot"].append(s); out["last_slot"].append(last); out["action"].append(-1 if dead else int(A[s]))
        out["dead"].append(bool(dead)); out["cls"].append(cls)
    dt = dict(reward=np.float32, done=np.uint8, steps=np.int32, first_slot=np.int32, last_slot=np.int32, action=np.int32, dead=bool)
    return {k: (np.array(v, dtype=dt[k]) if k in dt else v) for k, v in out.items()}


def staged(fx, ref):
    """the transitions a reference batch stages: (boards, action, reward, done, next boards), row for row"""
    f, l = ref["first_slot"], np.where(ref["dead"], ref["first_slot"], ref["last_slot"])
    return fx["S"][f], ref["action"], ref["reward"], ref["done"], fx["S2"][l]


def trajectory_walk(fx, slots, n, stride, gamma):
    """Independent of assemble(): walks the PUSH ORDER.  Transition t went to slot t % cap; its trajectory continues at t + stride, which
    exists iff it was pushed (t + stride < pushes).  Everything in fp64.  -> per row (R, m, D, last slot, dead)"""
    P, cap = fx["pushes"], fx["cap"]
    a, r, d = fx["push_A"], fx["push_R"].astype(np.float64), fx["push_D"]
    rows = []
    for s in slots:
        s = int(s)
        if s >= P:                                     # never written: an empty slot
            rows.append((0.0, 1, False, s, True, 0.0))
            continue
        t = s + (P - 1 - s) // cap * cap                # the last push that landed in slot s
        if a[t] < 0:
            rows.append((float(r[t]), 1, bool(d[t]), s, True, abs(float(r[t]))))
            continue
        Rs, mag, m, Dn, last, dead = float(r[t]), abs(float(r[t])), 1, bool(d[t]), s, False
        for k in range(1, n):
            if Dn:
                break
            u = t + k * stride
            if u >= P or a[u] < 0:
                dead = True
                break
            term = float(gamma) ** k * float(r[u])
            Rs += term; mag += abs(term)
            m, Dn, last = k + 1, bool(d[u]), u % cap
        rows.append((Rs, m, Dn, last, dead, mag))
    return rows


def reward_bound(n, mag):
    """|fl32 chain - fp64 sum|: (float)gamma is off by 2^-24 relative, so disc_k by (2k - 1) 2^-24; the product adds one rounding, the
    k-th running sum one more on everything summed so far: each term carries at most (2k + n) <= 3n roundings of 2^-24 relative, plus
    the second-order rest (factor 1.01)"""
    return 3 * n * 2.0 ** -24 * mag * 1.01


def random_boards(rng, count):
    """legal-to-push boards that are all different: 10 pieces of random codes 1..14 on random squares"""
    B = np.zeros((count, 90), np.uint8)
    for i in range(count):
        sq = rng.choice(90, size=10, replace=False)
        B[i, sq] = rng.integers(1, 15, size=10)
    return B


def fixture(cap, stride, pushes, seed, p_done=0.15, p_empty=0.06):
    """`pushes` transitions in push order into a ring of `cap`, and the ring's arrays as they stand afterwards"""
    rng = np.random.default_rng(seed)
    pA = rng.integers(0, 90, size=pushes).astype(np.int32)
    pA[rng.random(pushes) < p_empty] = -1
    pR = rng.uniform(-1.0, 1.0, size=pushes).astype(np.float32)
    pD = (rng.random(pushes) < p_done).astype(np.uint8)
    pS, pS2 = random_boards(rng, pushes), random_boards(rng, pushes)
    A = np.full(cap, -1, np.int32); R = np.zeros(cap, np.float32); D = np.zeros(cap, np.uint8)
    S = np.zeros((cap, 90), np.uint8); S2 = np.zeros((cap, 90), np.uint8)
    for t in range(pushes):
        A[t % cap], R[t % cap], D[t % cap], S[t % cap], S2[t % cap] = pA[t], pR[t], pD[t], pS[t], pS2[t]
    size = min(pushes, cap)
    return dict(cap=cap, stride=stride, pushes=pushes, seed=seed, size=size, write_pos=pushes % cap, A=A, R=R, D=D, S=S, S2=S2,
                push_A=pA, push_R=pR, push_D=pD, push_S=pS, push_S2=pS2)


# (capacity, stride, pushes, n the fixture is built for): a wrapped ring whose capacity is no multiple of the stride, a longer chain on
# a ring that wrapped three times, and a ring that is not full yet
FIXTURES = {"wrapped37": (37, 4, 50, 3), "wrapped40": (40, 4, 120, 5), "partial37": (37, 4, 30, 3)}
FIXTURE_SEEDS = {"wrapped37": 1, "wrapped40": 1, "partial37": 1}


def named_fixture(name):
    cap, stride, pushes, _ = FIXTURES[name]
    return fixture(cap, stride, pushes, FIXTURE_SEEDS[name])


def all_slots(fx):
    """the rows every test draws at least once: every slot of the ring, filled or not"""
    return np.arange(fx["cap"], dtype=np.int32)


def filled_slots(fx):
    """the identity batch: the filled part of the ring, in slot order"""
    return np.arange(fx["size"], dtype=np.int32)
