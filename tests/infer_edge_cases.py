"""The table of small inference calls that sit on the kernel-selection boundaries of the Q-net's forward paths (xq_dqn.hip, xq_l0.hip.h,
xq_apply.hip.h, xq_env.hip), shared by tests/test_infer_shape_edges_gpu.py (every case on the device against the fp64 rows of
batch_ref.q_rows) and the CPU controls of tests/test_batch_ref_cpu.py (the same cases: a damaged result must leave the bar).  Test
infrastructure only, in the style of tests/td_edge_cases.py.

The shape rules below restate the library's predicates as plain arithmetic on (layer sizes, n, n_out, precision); nothing here is
imported from the library, so a predicate that moves without its documentation fails the path assertions of the GPU test.  Where two
kernels share a bracket name and its arithmetic the comment says so and nothing is asserted.

Bars (none is new): fp32 rows from full layer-0 sums 5e-6 absolute (test_forward_matches_oracle), fp32 rows of the select chain produced
from derived sums 2e-5 (test_select_chain_layer0_sums_kept_between_plies), bf16 batch_ref.BF16_QTOL, the TD step batch_ref.TOLERANCES.
"""
from collections import namedtuple

import numpy as np

BAR_F32, BAR_DERIVED = 5e-6, 2e-5
ND_CYCLE = (0, 1, 2, 7, 8, 9, 40)          # squares that differ between two boards of a pair: both sides of "at most 8", 0 and 1, a reset

# kind: boards = xq_dqn_forward_boards_dev once; ldq = the same through the C ABI with ldq > n_out; select = xq_dqn_select_q_dev four
# times; collect = one xq_trainer_collect; dense = xq_dqn_forward; td = one td_update of rule 0
Case = namedtuple("Case", "family kind sizes n n_out prec wscale seed opt")


def _case(family, kind, net, n, n_out=96, prec=0, wscale=1.0, seed=0, **opt):
    return Case(family, kind, [1260] + [int(s) for s in net.split("-")], n, n_out, prec, wscale, seed, opt)


def _name(c):
    opt = "".join(f"_{k}{v if isinstance(v, str) else int(v)}" for k, v in sorted(c.opt.items()))
    return (f"{c.family}_{c.kind}_{'-'.join(str(s) for s in c.sizes[1:])}_n{c.n}_o{c.n_out}_p{c.prec}" + ("_w3" if c.wscale != 1.0 else "") + opt)


def _table():
    t = []
    # A. xq_dqn_forward_boards_dev, fp32.
    # head form (q_head): k-slabs + q_head_finish_kernel when n_out <= 96, n >= 2048 and Hl % 128 == 0, else the tile kernel's own
    # epilogue.  n = 2049 and 2080 leave a ragged last 64-row tile under force_small with slab_stride = n * nc; n_out = 90 gives nc = 92,
    # n_out = 1 gives nc = 4, 97 is the first count the plain head takes.  Both forms are bracketed gemm_q90_select / gemm_q_full with
    # 2 n n_out K flops: the brackets do not tell them apart, the fp64 rows do.
    for n in (2047, 2048, 2049, 2080):
        for n_out in (90, 96):
            t.append(_case("A", "boards", "128-8100", n, n_out, wscale=3.0 if (n, n_out) == (2049, 90) else 1.0))
    t.append(_case("A", "boards", "128-8100", 2048, 1))
    t.append(_case("A", "boards", "128-8100", 2048, 97))
    t.append(_case("A", "boards", "192-8100", 2048, 96))              # K % 128 != 0: the plain head
    t.append(_case("A", "ldq", "128-90", 2048, 90, ldq=96))           # make_player's call for a 90-output net: columns 90..95 stay untouched
    # hidden products (hidden_forward): n % 128 == 0, N % 128 == 0, K % 32 == 0 walk (gemm_fwd_persistent_kernel, one chain), anything
    # else the tile kernel; the walk takes 128 x 128 tiles from 512 tiles on (8192 x 1024: 512 | 8064 x 1024: 504 tiles of 64 x 128).
    # Walk and tile kernel share gemm_hidden_fwd and 2 n N K flops: not asserted.
    t.append(_case("A", "boards", "128-128-8100", 128))
    t.append(_case("A", "boards", "128-128-8100", 129))
    t.append(_case("A", "boards", "128-160-8100", 128))
    t.append(_case("A", "boards", "144-128-8100", 128))               # K % 32 != 0
    t.append(_case("A", "boards", "128-1024-8100", 8064))
    t.append(_case("A", "boards", "128-1024-8100", 8192))
    # layer-0 gather (l0_forward_kernel<false>, one wave per board, 4 boards per block): H % 4 != 0 takes scalar loads, H = 64 leaves
    # lanes of the float4 column loop idle, H = 320 takes its second trip (256 columns per trip); n = 1 and 5: a block with idle waves
    t.append(_case("A", "boards", "127-129-132-8100", 37))
    t.append(_case("A", "boards", "64-64-8100", 37))
    t.append(_case("A", "boards", "320-64-8100", 37))
    t.append(_case("A", "boards", "64-64-8100", 1))
    t.append(_case("A", "boards", "320-64-8100", 5, wscale=3.0))
    # B. xq_dqn_select_q_dev, fp32, four calls without a parameter update.
    # ride predicate (dqn_q90_boards): the head rides on the last hidden product (EPI_HEAD) iff n >= 2048, n % 64 == 0, Hl % 128 == 0,
    # L[nl-2] % 32 == 0, nout >= 128 and nl >= 3; one case per condition.  Riding: gemm_q90_select is q_head_finish_kernel alone
    # (n * 96 * slabs flops, slabs = Hl / 64) and gemm_hidden_fwd carries 2 n Hl 96 more; not riding: 2 n 96 Hl under gemm_q90_select.
    t.append(_case("B", "select", "128-128-8100", 2048))              # rides, 2 slabs
    t.append(_case("B", "select", "128-128-8100", 2047))              # n < 2048
    t.append(_case("B", "select", "128-128-8100", 2080))              # n % 64 != 0: slabbed head on a ragged tile
    t.append(_case("B", "select", "128-384-8100", 2048))              # 6 slabs
    t.append(_case("B", "select", "128-640-8100", 2048, wscale=3.0))  # 10 slabs: q_head_finish_kernel's third group of four is a pair
    t.append(_case("B", "select", "144-128-8100", 2048))              # L[nl-2] % 32 != 0: slabbed head
    t.append(_case("B", "select", "128-128-96", 2048))                # nout < 128
    t.append(_case("B", "select", "128-8100", 2048))                  # nl == 2
    # kept layer-0 sums (l0_select_kernel): the first call of an update period gathers in l0_forward_kernel, the second sums in full
    # and keeps z_1 and the board, later calls derive (at most 8 squares differ: take the old rows out, add the new ones; more: the
    # full sum again).  Between calls the boards are rewritten in place: row i differs on ND_CYCLE[(i + call) % 7] squares, with squares
    # that empty (a take-out row alone), fill (an add row alone) and change their piece.  The three forms show in the bytes of
    # l0_forward_gather.  Widths with H % 4 != 0 are never kept.  `drop`: apply_grads of a zero gradient, then a fifth call: the sums
    # must have been dropped, so it has the bits of xq_dqn_forward_boards_dev.
    t.append(_case("B", "select", "256-256-8100", 300, edit=1, drop=1))
    t.append(_case("B", "select", "128-128-8100", 2048, edit=1))
    t.append(_case("B", "select", "127-129-132-8100", 37, edit=1))
    # C. xq_trainer_collect at 2048 games, epsilon 0: the env kernel finishes the riding head from its k-slabs itself ((s0+s1)+(s2+s3)
    # per group of four: prefetched for <= 8 slabs, loaded late for more), or reads finished rows where nothing rides (128-8100).
    # overlap_collect = 1 puts the chain on the collect stream with 64 x 64 tiles (brackets "<name>@select").
    for ov in (0, 1):
        for hl in (128, 384, 512, 640, 1024):
            t.append(_case("C", "collect", f"128-{hl}-8100", 2048, 90, overlap=ov, wscale=3.0 if hl == 384 else 1.0))
        t.append(_case("C", "collect", "128-8100", 2048, 90, overlap=ov))
    t.append(_case("C", "collect", "128-640-8100", 2048, 90, overlap=1, versus=1))
    # D. bf16 Q-net (set_precision(1)), xq_dqn_forward_boards_dev and the select chain: the bf16 loop of its own at whole 256 x 128 x 64
    # tiles (hidden_bf16_dma_shape), the tile kernel on bf16 pairs otherwise; the head always the tile kernel on pairs; first hidden
    # layers outside wide_bf (96, 320: 512 % H != 0) take the narrow gather; ld % 4 != 0 the scalar loads.  All under the same brackets.
    for kind in ("boards", "select"):
        for n_out in ((90, 96) if kind == "boards" else (96,)):
            t.append(_case("D", kind, "256-256-8100", 256, n_out, prec=1))
            t.append(_case("D", kind, "256-256-8100", 300, n_out, prec=1, wscale=3.0 if n_out == 96 and kind == "boards" else 1.0))
            t.append(_case("D", kind, "256-192-256-8100", 256, n_out, prec=1))
            t.append(_case("D", kind, "96-128-8100", 300, n_out, prec=1))
            t.append(_case("D", kind, "320-128-8100", 300, n_out, prec=1))
            t.append(_case("D", kind, "100-132-8100", 37, n_out, prec=1))
    # E. dense xq_dqn_forward: launch_gemm takes 128 x 128 tiles once ceil(n / 128) * ceil(N / 128) >= 512 (897 x 8100: 8 * 64 | 896:
    # 448).  K = 1260 of the layer-0 product is no multiple of 32; the last 32 rows are uniform(-1, 1) instead of one-hot boards.
    # Tile sizes share their brackets: not asserted.
    t.append(_case("E", "dense", "64-8100", 896, 8100))
    t.append(_case("E", "dense", "64-8100", 897, 8100, wscale=3.0))
    # F. the s' chain of a TD step derived from the sums of s inside l0_forward_kernel (fp32 form; bf16: the 16-byte form, wide_bf
    # only).  (S, S2) differ on ND_CYCLE squares like the pairs of B.  Derived or gathered: one l0_forward_gather launch with the same
    # bytes either way, so each case runs again with derive off and both must meet check_q_y's bound of the one reference.
    t.append(_case("F", "td", "256-256-8100", 300, 8100, prec=0))
    t.append(_case("F", "td", "256-256-8100", 300, 8100, prec=1))
    t.append(_case("F", "td", "64-64-8100", 300, 8100, prec=0, wscale=3.0))
    out = {}
    for c in t:
        assert _name(c) not in out, _name(c)
        out[_name(c)] = c
    return out


CASES = _table()

# one case of each family for the CPU negative controls
CONTROL = ["A_boards_128-8100_n2049_o90_p0_w3", "B_select_128-640-8100_n2048_o96_p0_w3", "C_collect_128-384-8100_n2048_o90_p0_w3_overlap1",
           "D_boards_256-256-8100_n300_o96_p1_w3", "E_dense_64-8100_n897_o8100_p0_w3", "F_td_64-64-8100_n300_o8100_p0_w3"]


# ---- the shape rules ------------------------------------------------------------------------------------------------------------------
def head_slabbed(c, n_out=None):
    """q_head splits the head into k-slabs of 64 hidden columns (fp32 net)"""
    n_out = c.n_out if n_out is None else n_out
    return c.prec == 0 and n_out <= 96 and c.n >= 2048 and c.sizes[-2] % 128 == 0


def head_rides(c):
    """dqn_q90_boards: the select head rides on the last hidden product"""
    L, nl = c.sizes, len(c.sizes) - 1
    return c.prec == 0 and nl >= 3 and c.n >= 2048 and c.n % 64 == 0 and L[-2] % 128 == 0 and L[nl - 2] % 32 == 0 and L[-1] >= 128


def head_slabs(c):
    return c.sizes[-2] // 64


def sums_form(c, call):
    """layer 0 of select call `call` (1-based) of an update period, the handle fresh: "gather" (l0_forward_kernel), "kept" (full sum,
    z_1 kept), "derived" (from the kept sums)"""
    if c.prec != 0 or c.sizes[1] % 4 != 0 or call < 2:
        return "gather"
    return "kept" if call == 2 else "derived"


def l0_bytes(c, form):
    """the bytes one l0_forward_gather launch of one chain is bracketed with"""
    n, H = c.n, c.sizes[1]
    if form == "gather":
        return n * (48 + 32.0 * H * (2 if c.prec else 4) + H * 4)
    return n * (96 + (4.0 if form == "derived" else 32.0) * H * 4 + H * 12)


def hidden_flops(c, ride):
    L, nl = c.sizes, len(c.sizes) - 1
    return sum(2.0 * c.n * L[l + 1] * L[l] for l in range(1, nl - 1)) + (2.0 * c.n * L[-2] * 96 if ride else 0.0)


def head_flops(c, ride, n_out=None):
    n_out = c.n_out if n_out is None else n_out
    return float(c.n * 96 * head_slabs(c)) if ride else 2.0 * c.n * n_out * c.sizes[-2]


def hidden_walks(c, l):
    """hidden layer l (1-based product index) of one chain on the handle's stream takes the persistent walk; big: on 128 x 128 tiles"""
    N, K = c.sizes[l + 1], c.sizes[l]
    walk = c.prec == 0 and c.n % 128 == 0 and N % 128 == 0 and K % 32 == 0
    return walk, walk and (c.n // 128) * (N // 128) >= 512


def dense_big_tiles(c):
    return ((c.n + 127) // 128) * ((c.sizes[-1] + 127) // 128) >= 512


def bf16_own_loop(c, l):
    return c.prec != 0 and c.n % 256 == 0 and c.sizes[l + 1] % 128 == 0 and c.sizes[l] % 64 == 0


def wide_bf(c):
    H = c.sizes[1]
    return c.prec != 0 and H % 8 == 0 and ((H >= 512 and H % 512 == 0) or (H >= 64 and 512 % H == 0))


# ---- crafted board pairs ----------------------------------------------------------------------------------------------------------------
def edit_boards(boards, step, seed):
    """boards with row i changed on ND_CYCLE[(i + step) % 7] squares: squares that empty, squares that fill and pieces replaced by
    another, in turn (a single difference is each of the three somewhere); never more than 16 pieces of a colour.  Returns the new
    boards and the number of differing squares per row."""
    rng = np.random.default_rng(seed * 1000 + step)
    out = np.array(boards, dtype=np.uint8).reshape(-1, 90).copy()
    nds = np.zeros(len(out), np.int64)
    for i, b in enumerate(out):
        nd = ND_CYCLE[(i + step) % len(ND_CYCLE)]
        occ = list(rng.permutation(np.nonzero(b)[0]))
        emp = list(rng.permutation(np.nonzero(b == 0)[0]))
        kinds = [(j + i // len(ND_CYCLE) + step) % 3 for j in range(nd)]           # 0 empties, 1 fills, 2 another piece
        kinds.sort(key=lambda k: (k != 0, k != 2))                                  # take pieces off before any is put on
        for k in kinds:
            cnt = [int(((b >= 1) & (b <= 7)).sum()), int((b >= 8).sum())]
            if k != 1 and not occ:
                k = 1
            if k == 1 and (not emp or min(cnt) >= 16):
                k = 0
            if k == 0:
                b[occ.pop()] = 0
            elif k == 1:
                side = int(rng.integers(2))
                if cnt[side] >= 16:
                    side = 1 - side
                b[emp.pop()] = 1 + 7 * side + int(rng.integers(7))
            else:
                s = occ.pop()
                side = int(b[s] > 7)
                b[s] = 1 + 7 * side + (int(b[s]) - 1 - 7 * side + 1 + int(rng.integers(6))) % 7      # same colour, another type
        nds[i] = nd
    assert ((out != np.asarray(boards).reshape(-1, 90)).sum(axis=1) == nds).all()
    assert (((out >= 1) & (out <= 7)).sum(axis=1) <= 16).all() and ((out >= 8).sum(axis=1) <= 16).all() and out.max() <= 14
    return out, nds


# ---- the move checks of family C ---------------------------------------------------------------------------------------------------------
def move_checks(q, a, dests, bar, idle_ok=False):
    """The move checks of family C on fp64 rows q [n][90]: a[g] the destination game g played (-1: none), dests[g] its legal
    destinations; idle_ok: a game may have played nothing although it has moves (versus: it ended on the opponent's pre-move).  Returns (games whose fp64 best leads the runner-up by more than 2 bar, failures as text)."""
    clear, bad = 0, []
    for g in range(len(a)):
        ds = np.unique(dests[g])
        if len(ds) == 0 or a[g] < 0:
            if not (a[g] < 0 and (len(ds) == 0 or idle_ok)):
                bad.append(f"game {g}: action {a[g]} with {len(ds)} legal destinations")
            continue
        if a[g] not in ds:
            bad.append(f"game {g}: destination {a[g]} is not legal")
            continue
        v = np.sort(q[g, ds])[::-1]
        if q[g, a[g]] < v[0] - 2 * bar:
            bad.append(f"game {g}: Q {q[g, a[g]]:.9f} of the move played is {v[0] - q[g, a[g]]:.3e} under the best")
        if len(v) == 1 or v[0] - v[1] > 2 * bar:
            clear += 1
            if a[g] != ds[np.argmax(q[g, ds])]:
                bad.append(f"game {g}: clear best {ds[np.argmax(q[g, ds])]} not played ({a[g]})")
    return clear, bad
