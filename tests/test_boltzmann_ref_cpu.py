"""tests/boltzmann_ref.py, the definition of the Boltzmann pick, held to the analytic softmax, to an fp32 emulation of the device rule
and to negative controls, on the inputs tests/test_boltzmann_gpu.py runs the env kernel on (tests/boltzmann_edge_cases.py).  No GPU.

The band inside which a draw may resolve either way is derived in boltzmann_ref's docstring; here it is a CONDITION: at most 2 % of
the draws of a case may be undecided, and the emulation must agree with the reference on every other draw under three summation
orders.
"""
import numpy as np
import pytest

import boltzmann_edge_cases as be
import boltzmann_ref as bz

F32 = np.float32
NEG = -np.inf


# ---- the reference against the analytic softmax ---------------------------------------------------------------------------------------
def test_pick_frequencies_over_every_u_match_the_softmax():
    r2 = np.arange(1 << 24, dtype=np.uint64) << np.uint64(8)             # every value of u once
    rng = np.random.default_rng(5)
    for n, T in ((2, 1.0), (7, 0.25), (65, 0.05), (128, 4.0)):
        v = rng.uniform(-1.0, 1.0, n).astype(F32)
        idx, und = bz.pick_many(v, T, r2)
        freq = np.bincount(idx, minlength=n) / float(1 << 24)
        p = bz.softmax(v, T)
        # a boundary moves a move's count by at most one draw at either end
        assert np.abs(freq - p).max() <= 2.5 * 2.0 ** -24, (n, T, float(np.abs(freq - p).max()))
        assert und.mean() <= bz.MAX_UNDECIDED, (n, T, float(und.mean()))
        print(f"BOLTZMANN softmax n {n} T {T}: max |freq - p| {np.abs(freq - p).max():.3e}, undecided {und.mean():.5f}")


def test_a_large_temperature_is_near_uniform_and_a_small_one_is_the_first_maximum():
    rng = np.random.default_rng(6)
    v = rng.uniform(-1.0, 1.0, 40).astype(F32)
    r2 = rng.integers(0, 1 << 32, 200000, dtype=np.uint64)
    idx, _ = bz.pick_many(v, 1000.0, r2)
    freq = np.bincount(idx, minlength=40) / len(r2)
    assert np.abs(freq - 1 / 40).max() < 0.003, freq                     # weights within e^(+-0.002) of each other; 3 sigma of the count
    v[17] = F32(1.5)                                                     # a unique maximum, 0.5 ahead: e^-500 at T = 1e-3
    idx, und = bz.pick_many(v, 1e-3, r2)
    assert (idx == 17).all() and bz.first_max(v) == 17
    assert und.mean() < 1e-3


def test_where_the_maximum_is_not_finite_the_first_maximum_rule_applies():
    r2 = np.random.default_rng(7).integers(0, 1 << 32, 1000, dtype=np.uint64)
    inf, nan = F32(np.inf), F32(np.nan)
    for v, want in (([NEG, NEG, NEG], 0), ([0.1, inf, 0.5, inf], 1), ([NEG, 0.2, inf], 2)):
        idx, und = bz.pick_many(np.array(v, F32), 0.25, r2)
        assert (idx == want).all() and not und.any(), v
    # a NaN counts as -inf: never picked; all NaN: entry 0
    codes = np.arange(4)
    q = np.zeros(90, F32)
    q[:4] = [nan, 0.3, nan, 0.1]
    v = bz.values(q, codes)
    idx, _ = bz.pick_many(v, 1.0, r2)
    assert set(idx.tolist()) == {1, 3}
    q[:4] = nan
    assert (bz.pick_many(bz.values(q, codes), 1.0, r2)[0] == 0).all()
    # -inf never wins beside finite values, wherever it stands
    idx, _ = bz.pick_many(np.array([NEG, 0.0, NEG, 0.0, NEG], F32), 4.0, r2)
    assert set(idx.tolist()) == {1, 3}
    # the rule's `explored`: 1 on the epsilon branch (move r1 mod n), 2 where the draw left the first maximum
    q = np.linspace(-1, 1, 90).astype(F32)
    codes = np.array([5, 80, 40], np.uint16)
    assert bz.step(q, codes, 1.0, [0, 7, 0, 0], eps_u32=1) == (1, 1, False)
    assert bz.step(q, codes, 1.0, [5, 7, 0, 0], eps_u32=1)[:2] == (0, 2)             # u = 0: the first entry, not the maximum
    assert bz.step(q, codes, None, [5, 7, 0, 0], eps_u32=1) == (1, 0, False)
    assert bz.step(q, codes, 1.0, [5, 7, 0, 0], eps_u32=1, swap=True)[:2] == (0, 0)  # under the swap entry 0 reads q[85], the maximum


# ---- an fp32 emulation of the device rule ------------------------------------------------------------------------------------------------
def _scan_sequential(W):
    return np.cumsum(W, axis=1, dtype=F32)


def _scan_pairwise(W):
    """Hillis-Steele over all 128 entries: every step adds the entry 2^k to the left"""
    C = W.copy()
    k = 1
    while k < C.shape[1]:
        S = C.copy()
        S[:, k:] = (C[:, k:] + C[:, :-k]).astype(F32)
        C, k = S, 2 * k
    return C


def _scan_wave(W64):
    """the wave's network on 64 lanes: shifts by 1, 2, 4, 8 inside rows of 16, then lane 15 into row 1 and lane 47 into row 3, then lane
    31 into rows 2 and 3"""
    C = W64.copy()
    for k in (1, 2, 4, 8):
        S = C.copy()
        for row in range(4):
            lo = 16 * row
            S[:, lo + k:lo + 16] = (C[:, lo + k:lo + 16] + C[:, lo:lo + 16 - k]).astype(F32)
        C = S
    S = C.copy()
    S[:, 16:32] = (C[:, 16:32] + C[:, 15:16]).astype(F32)
    S[:, 48:64] = (C[:, 48:64] + C[:, 47:48]).astype(F32)
    C = S.copy()
    C[:, 32:64] = (S[:, 32:64] + S[:, 31:32]).astype(F32)
    return C


def _scan_halves(W):
    """lanes 0..63 scan moves 0..63; a second scan of moves 64..127 is offset by the first total"""
    a = _scan_wave(W[:, :64])
    b = (_scan_wave(W[:, 64:]) + a[:, 63:64]).astype(F32)
    return np.concatenate([a, b], axis=1)


SCANS = {"sequential": _scan_sequential, "pairwise": _scan_pairwise, "64 + 64 with offset": _scan_halves}


def emulate(V, T, r2, scan, subtract_max=True, strict=True):
    """the device rule in np.float32 on padded candidate vectors V [G][128] -> picks [G] (-1 where the first-maximum rule applies)"""
    it = bz.inv_temperature(T)
    m = V.max(axis=1, keepdims=True)
    finite = np.isfinite(m[:, 0])
    with np.errstate(invalid="ignore", over="ignore"):
        d = (V - (m if subtract_max else F32(0))).astype(F32)
        x = (d * it).astype(F32)
        W = np.where(V == NEG, F32(0), np.exp(x).astype(F32)).astype(F32)
        C = scan(W)
        total = C[:, -1]
        u = ((np.asarray(r2, dtype=np.uint64) >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)
        t = (u * total).astype(F32)[:, None]
        hit = (W > 0) & ((C > t) if strict else (C >= t))
    first = np.where(hit.any(axis=1), hit.argmax(axis=1), 127 - (W > 0)[:, ::-1].argmax(axis=1))
    return np.where(finite, first, -1)


@pytest.mark.parametrize("T", be.TEMPS)
def test_fp32_emulation_agrees_on_every_decided_draw_and_few_are_undecided(T):
    V, n_of = be.candidate_vectors()
    want = be.expected(T)
    R = be.philox_words()
    share = want["undecided"][n_of > 0].mean()
    print(f"BOLTZMANN shared inputs T {T}: undecided {share:.5f}, draws that leave the first maximum {np.mean(want['explored'] == 2):.3f}")
    assert share <= bz.MAX_UNDECIDED, share
    for name, scan in SCANS.items():
        got = emulate(V, T, R[:, 2], scan)
        live = (n_of > 0) & (got >= 0)
        bad = np.nonzero(live & ~want["undecided"] & (got != want["idx"]))[0]
        moved = int((live & (got != want["idx"])).sum())
        print(f"  {name}: {moved} undecided draws resolved the other way")
        assert len(bad) == 0, (name, T, [(int(g), be.inputs()["pattern"][g], int(got[g]), int(want["idx"][g])) for g in bad[:8]])
        # where the first-maximum rule applies the reference says so too
        fm_rule = (n_of > 0) & (got < 0)
        assert (want["explored"][fm_rule] == 0).all()


def test_the_shared_inputs_cover_their_edges():
    inp = be.inputs()
    n_of = np.array([len(c) for c in inp["lists"]])
    for length in be.SPECIAL_LENGTHS + (inp["longest"],):
        names = {inp["pattern"][g] for g in np.nonzero(n_of == length)[0]}
        assert len(names) >= (1 if length == 0 else 4), (length, names)
    assert (n_of > 64).sum() >= 40
    used = set(inp["pattern"])
    assert used >= {"tie_all", "zeros_signed_minus_first", "inf_pos", "nan_all", "neginf_all", "inf_neg_rest", "wide", "uniform"}, used
    # every temperature leaves the first maximum often and stays on it often: both values of `explored` are tested
    for T in be.TEMPS:
        e = be.expected(T)["explored"][n_of > 1]
        assert 0.02 < np.mean(e == 2) < 0.98, (T, float(np.mean(e == 2)))


# ---- negative controls: a wrong rule must move picks on the shared inputs -----------------------------------------------------------------
def _reference_picks(V, n_of, T, r2):
    out = np.full(len(V), -1)
    for g in np.nonzero(n_of > 0)[0]:
        out[g] = bz.pick(V[g, :n_of[g]], T, int(r2[g]))[0]
    return out


def test_control_no_max_subtraction_breaks_on_large_values():
    V, n_of = be.candidate_vectors()
    T = 0.05
    want = be.expected(T)
    got = emulate(V, T, be.philox_words()[:, 2], _scan_sequential, subtract_max=False)
    wide = np.array([p == "wide" for p in be.inputs()["pattern"]]) & (n_of > 1) & ~want["undecided"]
    moved = int((got[wide] != want["idx"][wide]).sum())
    print(f"no max subtraction: {moved} of {int(wide.sum())} decided draws on rows outside [-1, 1] move")
    assert moved >= 0.25 * wide.sum(), (moved, int(wide.sum()))


def test_control_word_1_instead_of_word_2():
    V, n_of = be.candidate_vectors()
    R = be.philox_words()
    for T in (0.25, 1.0):
        want = be.expected(T)
        got = _reference_picks(V, n_of, T, R[:, 1])
        live = (n_of > 1) & ~want["undecided"]
        moved = float((got[live] != want["idx"][live]).mean())
        print(f"word 1 for word 2, T {T}: {moved:.3f} of the decided draws move")
        assert moved >= 0.2, moved


def test_control_greater_or_equal_in_the_pick():
    """`>=` for `>` moves a draw only where t stands on a prefix sum exactly — an undecided draw for the band, so the device cannot
    be held to it; the reference can: on words that put u on 0, 1/4, 1/2, 3/4"""
    V, n_of = be.candidate_vectors()
    moved = total = 0
    for r2 in be.CRAFTED_R2:
        words = np.full(len(V), r2, np.uint64)
        want = _reference_picks(V, n_of, 1.0, words)
        got = emulate(V, 1.0, words, _scan_sequential, strict=False)
        live = (n_of > 1) & (got >= 0)
        moved += int((got[live] != want[live]).sum())
        total += int(live.sum())
    print(f">= for >: {moved} of {total} crafted draws move")
    assert moved >= 50, moved


def test_control_temperature_on_the_epsilon_branch():
    inp, R = be.inputs(), be.philox_words()
    T = 1.0
    want = be.expected(T, eps=be.EPS_COMPOSED)
    eps_u32 = int(be.EPS_COMPOSED * 4294967296.0)
    moved = n_eps = 0
    for g, codes in enumerate(inp["lists"]):
        if len(codes) > 1 and int(R[g, 0]) < eps_u32:
            n_eps += 1
            assert want["explored"][g] == 1 and want["idx"][g] == int(R[g, 1]) % len(codes)
            wrong = bz.step(inp["q"][g], codes, T, R[g], 0)[0]           # the draw where the uniform index belongs
            moved += wrong != want["idx"][g]
    print(f"temperature on the epsilon branch: {moved} of {n_eps} epsilon plies move")
    assert 0.25 * len(inp["lists"]) < n_eps < 0.35 * len(inp["lists"]) and moved >= 0.5 * n_eps, (moved, n_eps)


@pytest.mark.parametrize("T", be.TEMPS)
def test_few_draws_are_undecided_under_the_view_and_with_epsilon(T):
    n_of = np.array([len(c) for c in be.inputs()["lists"]])
    for kw in (dict(q_view=True), dict(eps=be.EPS_COMPOSED)):
        share = be.expected(T, **kw)["undecided"][n_of > 0].mean()
        assert share <= bz.MAX_UNDECIDED, (T, kw, share)
