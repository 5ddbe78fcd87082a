"""The table of worst-case inputs of the screened max pass, shared by tests/test_screen_worst_case_gpu.py (four or five device steps per
case against fp64) and tests/test_screen_ref_cpu.py (the same cases through the numpy model of tests/screen_ref.py: the depth, the
candidate counts and the negative controls).  Test infrastructure only; nothing is imported from the library.

Every case has 8100 outputs and a batch at which the screen runs (64 x ceil(n / 128) >= 512 tiles: n >= 897).  Families:
  a. width x path: Hl = 128 and 960 (the tile kernel's CM_TOP2 mode and qmax_refine_kernel<0, *>; 960 is the widest last hidden layer a TD
     step takes — its output-gradient kernel refuses 1024, which the screen itself would take: CPU_ONLY below), Hl = 256 with the TD arithmetic riding
     (qmax_refine2_kernel<256, true>), with Huber on (<256, true, HuberLoss>), with set_td_tail(False) (<256>), and Hl = 512 (<512>); n = 1024
     and 1100 (ragged sample panel), for Hl = 256 also 897, the least batch the screen takes.
  b. where the two rows sit, both orders of (j*, rival): (4321, 17); (8099, 8064): the last real row, in the padded chunk — both lie in group
     252, so this pair is a whole-group case like (200, 201); (8099, 8068): the same chunk, two groups; (0, 95): the ends of the dynamic rows;
     (40, 70) with rows >= 96 at a tenth of the norm, so that the dynamic slot alone carries the bound; (200, 201): one group.  The full cross
     of pairs and orders at Hl = 256, with the selecting net and the producer of the activation operand alternating over it; one pair each at
     the other widths.
  c. the selecting net: td_net = 1 on both producers at Hl = 256 and once at every other width (family a runs td_net = 0).
  d. one biased case per width: z ~ 0.05 .. 0.09 through output biases of +0.05 on the two rows and -0.01 .. -0.06 elsewhere.
"""
from screen_ref import Case, group_of

PAIRS = [(4321, 17), (8099, 8064), (8099, 8068), (0, 95), (40, 70), (200, 201)]


def _case(family, Hl, n, net, pair=(4321, 17), td_net=0, tail=True, huber=False, biased=False):
    return Case(family, Hl, n, net, pair[0], pair[1], td_net, tail, huber, biased, low_static=set(pair) == {40, 70})


def name_of(c):
    sw = ("" if c.tail else "_notail") + ("_huber" if c.huber else "") + ("_biased" if c.biased else "")
    return f"{c.family}_{c.net}_{c.Hl}_n{c.n}_j{c.jstar}_J{c.rival}_net{c.td_net}{sw}"


def one_group(c):
    """the two rows share a 32-row group: the whole-group rule has to fire"""
    return group_of(c.jstar) == group_of(c.rival)


def expected_counts(c):
    """(candidate groups, whole groups) per sample"""
    return (1, 1) if one_group(c) else (2, 0)


def _table():
    t = []
    nets = ("gather", "product")
    # a. width x path
    for i, Hl in enumerate((128, 960, 512)):
        for j, n in enumerate((1024, 1100)):
            t.append(_case("a", Hl, n, nets[(i + j) & 1]))
    for k, sw in enumerate((dict(), dict(huber=True), dict(tail=False))):
        for j, n in enumerate((1024, 1100, 897)):
            t.append(_case("a", 256, n, nets[(k + j) & 1], **sw))
    # b. where the two rows sit
    i = 0
    for pair in PAIRS:
        for p in (pair, pair[::-1]):
            t.append(_case("b", 256, 1100, nets[i & 1], p, td_net=(i >> 1) & 1))
            i += 1
    t.append(_case("b", 128, 1100, "product", (0, 95)))
    t.append(_case("b", 128, 1024, "gather", (201, 200)))
    t.append(_case("b", 512, 1100, "gather", (200, 201)))
    t.append(_case("b", 512, 1024, "product", (70, 40)))
    t.append(_case("b", 960, 1100, "gather", (8064, 8099)))
    t.append(_case("b", 960, 1024, "product", (8068, 8099)))
    # c. the selecting net
    t.append(_case("c", 256, 1024, "gather", td_net=1))
    t.append(_case("c", 256, 1100, "product", td_net=1))
    t.append(_case("c", 128, 1100, "gather", td_net=1))
    t.append(_case("c", 512, 1024, "product", td_net=1))
    t.append(_case("c", 960, 1100, "product", td_net=1))
    # d. biased
    t.append(_case("d", 128, 1100, "gather", biased=True))
    t.append(_case("d", 256, 1100, "product", biased=True, td_net=1))
    t.append(_case("d", 512, 1100, "gather", biased=True))
    t.append(_case("d", 960, 1024, "product", biased=True))
    cases = {name_of(c): c for c in t}
    assert len(cases) == len(t)
    return cases


CASES = _table()
# K = 1024, the widest product the screen's bound is stated for (the largest accumulation term): through the CPU model only
CPU_ONLY = {name_of(c): c for c in (_case("cpu", 1024, 1024, "gather"), _case("cpu", 1024, 1024, "product", (201, 200), biased=True))}


def case(name):
    return CASES[name] if name in CASES else CPU_ONLY[name]


def constructions():
    """one case per distinct output layer: the CPU model does not depend on n, the hidden layers that produce the activations, the
    selecting net or the handle's switches"""
    seen = {}
    for name, c in list(CASES.items()) + list(CPU_ONLY.items()):
        seen.setdefault((c.Hl, c.jstar, c.rival, c.biased, c.low_static), name)
    return sorted(seen.values(), key=lambda s: case(s).Hl)
