"""CPU checks of the legal-move TD bootstrap (not gpu): tests/legal_ref.py's move lists against the REAL reference engine's lists of
tests/golden/ref_bigmoves.npz and ref_sparse.npz for both colours, known answers of the rule (with the all-outputs rule as the negative
control), the winner on ties, signed zeros, infinities and NaN against tests/first_max.py in move-list order, the mirror symmetry, the
near-tie condition the GPU test's flip allowance rests on, and header, ctypes table, library and work model agreeing on the new entry
points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import argmax_edge_cases as ac
import batch_ref as br
import first_max as fm
import legal_ref as lr
import mirror_ref as mr
import xqoracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_dqn_set_td_bootstrap", "xq_dqn_get_td_bootstrap", "xq_dqn_td_grads_sided", "xq_dqn_td_update_host_sided",
               "xq_dqn_last_legal", "xq_replay_track_next_player", "xq_replay_push_host_sided", "xq_replay_get_next_player",
               "xq_trainer_set_td_bootstrap")
SMALL_NET = [1260, 64, 64, 8100]
NET_SEED = 7                                    # the seed tests/test_legal_gpu.py gives its nets
GAMMA = 0.97


# ---- the move lists rest on the real engine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_boards,long_lists,empty", [("ref_bigmoves.npz", 160, (71, 89), (0, 0)), ("ref_sparse.npz", 730, None, (20, 20))])
def test_move_lists_are_the_reference_engines_for_both_colours(golden_dir, name, n_boards, long_lists, empty):
    boards, sides, lists = lr.fixture_rows(golden_dir, name)
    assert len(boards) == 2 * n_boards
    for b, s, want in zip(boards, sides, lists):
        got = lr.move_list(b, s)
        assert got.dtype == np.uint16 and np.array_equal(got, want)
    for c in (0, 1):
        mine = lists[c::2]
        if long_lists is not None:              # both registers of the two-register pick
            assert sum(len(x) > 64 for x in mine) == long_lists[c] and max(len(x) for x in mine) == (76, 77)[c]
        assert sum(len(x) == 0 for x in mine) == empty[c]


# ---- known answers -----------------------------------------------------------------------------------------------------------------------
def bias_only_net(bias):
    """1260-8-8100 with every weight 0: z(s') is the output bias whatever the board"""
    sizes = [1260, 8, 8100]
    nw, nb = xo.nn_counts(sizes)
    b = np.zeros(nb)
    b[8:] = bias
    return br.Net(sizes, np.zeros(nw), b)


def known_rows(golden_dir):
    boards, sides, lists = lr.fixture_rows(golden_dir, "ref_sparse.npz")
    live = [i for i, x in enumerate(lists) if 0 < len(x)]
    i = next(k for k in live if len(set(int(c) % 90 for c in lists[k])) < 80)
    empty = next(k for k, x in enumerate(lists) if len(x) == 0)
    return boards, sides, lists, i, empty


def test_the_rule_ignores_outputs_no_move_reaches_and_the_all_outputs_rule_does_not(golden_dir):
    boards, sides, lists, i, empty = known_rows(golden_dir)
    reach = sorted(set(int(c) % 90 for c in lists[i]))
    unreachable = next(s for s in range(90) if s not in reach)
    bias = np.full(8100, -2.0)
    bias[5000] = 3.0                            # the largest z of all: an output >= 90
    bias[unreachable] = 1.0                     # the largest of 0..89: a square the side cannot reach
    bias[reach] = -1.0
    net = bias_only_net(bias)
    rows = [i, i, empty]
    S2, side = boards[rows], sides[rows]
    A, R, D = np.array([3, 3, 3]), np.array([0.25, 0.25, -0.5]), np.array([0, 1, 0])
    f = lr.forward(net, S2, S2, A, R, D, side, GAMMA)
    want = 0.25 + GAMMA * np.tanh(-1.0)
    assert abs(f.y[0] - want) < 1e-15 and f.astar[0] == int(lists[i][0]) % 90 and f.n_moves[0] == len(lists[i])
    assert f.y[1] == 0.25 and f.n_moves[1] == -1 and f.astar[1] == -1           # done: y = r
    assert f.y[2] == -0.5 and f.n_moves[2] == 0 and f.astar[2] == -1            # no move: y = r
    # negative control: the all-outputs rule fails the legal expectation, by more than 0.5
    y_all = lr.all_outputs_y(net, S2, R, D, GAMMA)
    assert abs(y_all[0] - (0.25 + GAMMA * np.tanh(3.0))) < 1e-15
    assert abs(y_all[0] - f.y[0]) > 0.5 and abs(y_all[0] - want) > 0.5
    assert y_all[1] == 0.25 and abs(y_all[2] - (-0.5)) > 0.5                    # ... and gives a side without a move a bootstrap
    # the second-best rule a reader might expect — the maximum over outputs 0..89 — fails it too
    assert abs((0.25 + GAMMA * np.tanh(1.0)) - f.y[0]) > 0.5


def test_double_rule_evaluates_the_online_pick_on_the_target_net(golden_dir):
    boards, sides, lists, i, _ = known_rows(golden_dir)
    tos = [int(c) % 90 for c in lists[i]]
    on, tg = np.full(8100, -2.0), np.full(8100, 0.1)
    on[tos[-1]] = 0.5                           # online: the LAST entry's square wins
    tg[tos[0]], tg[tos[-1]] = 2.0, -0.3         # target: its own maximum is elsewhere
    assert tos[0] != tos[-1]
    net, tnet = bias_only_net(on), bias_only_net(tg)
    one = lambda rule: lr.forward(net, boards[[i]], boards[[i]], [5], [0.0], [0], sides[[i]], GAMMA, rule, target=tnet)
    assert abs(one(0).y[0] - GAMMA * np.tanh(0.5)) < 1e-15
    assert abs(one(1).y[0] - GAMMA * np.tanh(2.0)) < 1e-15 and one(1).astar[0] == tos[0]
    assert abs(one(2).y[0] - GAMMA * np.tanh(-0.3)) < 1e-15 and one(2).astar[0] == tos[-1]


@pytest.mark.parametrize("pattern", list(ac.Q_PATTERNS))
def test_winner_follows_the_first_maximum_rule_in_list_order(golden_dir, pattern):
    _, _, big = lr.fixture_rows(golden_dir, "ref_bigmoves.npz")
    _, _, sparse = lr.fixture_rows(golden_dir, "ref_sparse.npz")
    lists = big + sparse[:200]
    q, ok = ac.q_rows(pattern, lists, seed=3)
    assert ok.sum() >= (20 if pattern in ac.LONG_LIST_ONLY else 200)
    a, zm = lr.pick_rows(q, lists)
    not_lowest = 0
    for g, codes in enumerate(lists):
        if len(codes) == 0:
            assert a[g] == -1 and zm[g] == 0
            continue
        want = int(codes[fm.pick(q[g], codes)]) % 90
        assert a[g] == want, (pattern, g)
        assert zm[g:g + 1].view(np.uint32)[0] == q[g, want:want + 1].view(np.uint32)[0]
        not_lowest += want != min(int(c) % 90 for c in codes)
    if pattern == "tie_all":                    # list order, not square order: the first entry rarely reaches the lowest square
        assert not_lowest > len(lists) // 2


# ---- mirror ------------------------------------------------------------------------------------------------------------------------------
def reflected_net(sizes, w, b):
    """the net whose layer-0 input (square, piece) and whose outputs 0..89 are those of (row, 8 - col)"""
    w, b = np.array(w, dtype=np.float64), np.array(b, dtype=np.float64)
    net = br.Net(sizes, w, b)
    sq = mr.mirror_action(np.arange(90)).astype(np.int64)
    cols = (sq[:, None] * 14 + np.arange(14)[None, :]).reshape(-1)           # input j = s * 14 + p  ->  mirror(s) * 14 + p
    W0 = np.empty_like(net.W[0]); W0[:, cols] = net.W[0]
    Wo, Bo = net.W[-1].copy(), net.B[-1].copy()
    Wo[sq], Bo[sq] = net.W[-1][:90], net.B[-1][:90]
    w[:W0.size] = W0.reshape(-1)
    w[net.wo[-1]:] = Wo.reshape(-1)
    b[net.bo[-1]:] = Bo
    return br.Net(sizes, w, b)


def test_reflected_row_on_the_reflected_net_has_the_same_target(golden_dir):
    boards, sides, lists = lr.fixture_rows(golden_dir, "ref_sparse.npz")
    rows = np.arange(0, len(boards), 7)
    w, b = xo.init_weights(SMALL_NET, NET_SEED)
    b = np.random.default_rng(5).uniform(-0.05, 0.05, size=len(b))
    net, rnet = br.Net(SMALL_NET, w, b), reflected_net(SMALL_NET, w, b)
    n = len(rows)
    rng = np.random.default_rng(6)
    A, R, D = rng.integers(0, 90, n), rng.uniform(-1, 1, n), rng.random(n) < 0.1
    S2 = boards[rows]
    f = lr.forward(net, S2, S2, A, R, D, sides[rows], GAMMA)
    g = lr.forward(rnet, mr.reflect(S2), mr.reflect(S2), mr.mirror_action(A), R, D, sides[rows], GAMMA)
    assert (f.n_moves > 0).sum() > 150 and (f.n_moves == 0).any() and (f.n_moves == -1).any()
    assert np.array_equal(f.n_moves, g.n_moves)
    assert np.abs(f.y - g.y).max() < 1e-12 and np.abs(f.q - g.q).max() < 1e-12
    assert np.array_equal(mr.mirror_action(f.astar), g.astar)                # (-1 stays -1)
    assert not np.allclose(f.y, lr.forward(net, mr.reflect(S2), mr.reflect(S2), A, R, D, sides[rows], GAMMA).y)


# ---- near ties: the condition the GPU test's flip allowance rests on ---------------------------------------------------------------------
def test_few_rows_have_more_than_one_candidate_for_the_gpu_tests_net(golden_dir):
    w, b = xo.init_weights(SMALL_NET, NET_SEED)
    net = br.Net(SMALL_NET, w, b)
    many = rows_seen = 0
    gaps = []
    for name in ("ref_bigmoves.npz", "ref_sparse.npz"):
        boards, sides, lists = lr.fixture_rows(golden_dir, name)
        n = len(boards)
        f = lr.forward(net, boards, boards, np.zeros(n, int), np.zeros(n), np.zeros(n, int), sides, GAMMA, lists=lists)
        for i in np.flatnonzero(f.n_moves > 0):
            rows_seen += 1
            many += len(f.cands[i]) > 1
            z = np.sort(np.unique(f.z96[i, np.asarray(lists[i], dtype=np.int64) % 90]))
            if len(z) > 1:
                gaps.append(z[-1] - z[-2])
    print("rows", rows_seen, "with > 1 candidate", many, "gap < 1e-4", int((np.array(gaps) < 1e-4).sum()), "median gap", float(np.median(gaps)))
    assert rows_seen == 1740
    assert many <= br.MAX_FLIP_FRACTION[br.PRECISION_F32] * rows_seen


# ---- the entry points --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_legal_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_LEGAL, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_LEGAL) == set(NEW_SYMBOLS)
    assert (capi.BOOTSTRAP_ALL, capi.BOOTSTRAP_LEGAL) == (0, 1) and re.search(r"XQ_BOOTSTRAP_ALL = 0, XQ_BOOTSTRAP_LEGAL = 1", text)


def test_legal_on_a_null_handle_fails_loudly(capi):
    """no device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message"""
    k = C.c_int32()
    one = (C.c_uint8 * 90)()
    calls = [("xq_dqn_set_td_bootstrap", (None, 1)), ("xq_dqn_get_td_bootstrap", (None, C.byref(k))),
             ("xq_dqn_td_grads_sided", (None,) * 8 + (1, 0, 0)),
             ("xq_dqn_td_update_host_sided", (None, 1, one, one, None, None, None, None, 0, 0, 0.0, 1.0, None, None)),
             ("xq_dqn_last_legal", (None, 1, None, None, None, None)), ("xq_replay_track_next_player", (None,)),
             ("xq_replay_push_host_sided", (None, 1, one, None, None, None, one, one)),
             ("xq_replay_get_next_player", (None, 0, 1, one)), ("xq_trainer_set_td_bootstrap", (None, 1))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and ("null" in str(e.value).lower() or "bad argument" in str(e.value)), name


def build_legal_facade_probe():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "tests", "cpp", "legal_facade.cpp"), os.path.join(BUILD, "legal_facade"))


def test_legal_facade_probe_compiles(capi):
    """xq::TdBootstrap and xq::DQN::setTdBootstrap / tdBootstrap with plain g++ (no HIP headers)"""
    assert os.path.exists(build_legal_facade_probe())


def test_work_model_knows_the_legal_brackets_only_when_asked():
    import cn_chess_ai_amd.workmodel as wm
    cfg = ((1260, 256, 256, 8100), 8192, 8192)
    base, same, on = wm.step_work(*cfg), wm.step_work(*cfg, bootstrap="all"), wm.step_work(*cfg, bootstrap="legal")
    assert base == same and "legal_qmax" not in base and "gemm_legal_head" not in base
    assert set(on) - set(base) == {"legal_qmax", "gemm_legal_head", "td_target_delta"}
    assert set(base) - set(on) == {"gemm_qmax_screen", "qmax_refine"}
    assert on["legal_qmax"]["hbm_bytes"] == 8192 * (48 + 6 + 384 * 4 + 384 + 12) and on["legal_qmax"]["bound"] == "hbm"
    assert on["gemm_legal_head"]["flops"] == 2.0 * 8192 * 96 * 256
    dbl = wm.step_work(*cfg, bootstrap="legal", td="double")
    assert dbl["legal_qmax"]["hbm_bytes"] == 8192 * (48 + 6 + 384 * 8 + 384 + 12) and "colmax_reduce" not in dbl
    full = wm.step_work(*cfg, screened=False)
    assert set(wm.step_work(*cfg, bootstrap="legal", screened=False)) - set(full) == {"legal_qmax", "gemm_legal_head"}
    assert wm.rocprof_kernel("legal_qmax", *cfg[:2]) == "legal_qmax_kernel("
    assert "legal_side_stage" not in on and "legal_side_stage" not in wm.step_work(*cfg, mirror=True, n_step=3)
    for kw in (dict(mirror=True), dict(n_step=3), dict(n_step=3, mirror=True)):
        st = wm.step_work(*cfg, bootstrap="legal", **kw)
        assert st["legal_side_stage"]["hbm_bytes"] == 6.0 * 8192 and set(st) - set(wm.step_work(*cfg, bootstrap="legal")) >= {"legal_side_stage"}
    with pytest.raises(ValueError):
        wm.step_work(*cfg, bootstrap="legal", bf16=True)
    with pytest.raises(ValueError):
        wm.step_work(*cfg, bootstrap="some")
