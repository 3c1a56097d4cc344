"""The harness of the MMTM kernel tests (mmtmref.py) and the CPU-side conditions of
test_gpu_mmtm_forms.py: every exact case is exact (fp64 against integer or rational arithmetic on the
case's operands), the bf16 expected outputs are mostly inexact before the store and hold planted ties,
every mutant changes or violates at least 1 % of the checked outputs or is listed in NOT_CHECKED, the
bounded references summed in fp32 stay inside their own bounds, and the restated launch plans agree
with the library where it exposes them (gm_spatial_reduce_scratch) and reach every label.  No GPU."""
from fractions import Fraction

import pytest
import torch

import exactint as X
import mmtmref as M

DTYPES = ["bf16", "f32"]


# ---- launch plans ---------------------------------------------------------------------------------------

def test_plan_reaches_what_the_cases_name():
    p = M.nhwc_plan(64, 700, 1, 2)
    assert (p.S, p.hw_per, p.last) == (11, 64, 60)
    p = M.nhwc_plan(128, 784, 3, 2)
    assert (p.S, p.hw_per, p.last, p.ppt_full, p.ppt_last) == (22, 36, 28, (2, 3), (1, 2))
    p = M.nhwc_plan(128, 341, 64, 2)
    assert (p.S, p.ppi, p.ppt_full) == (1, 16, (21, 22)) and M.trips(21, 16) == (1, 1, 1)
    for dtype, C, R in (("bf16", 24, 10), ("bf16", 40, 6), ("f32", 12, 21)):
        p = M.nhwc_plan(C, 300, 2, M.ES[dtype])
        assert p.R == R and p.idle > 0 and R & (R - 1)               # idle lanes, R not a power of two
    for dtype, C in (("bf16", 2048), ("f32", 1024)):
        p = M.nhwc_plan(C, 7, 2, M.ES[dtype])
        assert (p.ncs, p.cw * M.ES[dtype], p.R, p.ppi) == (1, 4096, 1, 1)
        assert M.nhwc_plan(2 * C, 6, 2, M.ES[dtype]).ncs == 2
    for dtype in DTYPES:
        for nth in (256, 1024):
            plan = lambda name: [M.nhwc_plan(q["C"], q["HW"], M.col_problems(name, dtype)[0], M.ES[dtype], nth)  # noqa: E731
                                 for q in M.col_problems(name, dtype)[1]]
            assert [q.S > 1 for q in plan("mixedS")] == [True, False]
            assert len({(q.cw, q.S, q.ppi) for q in plan("four")}) == 4
            for name in ("split11", "split22"):
                q = plan(name)[0]
                assert q.S > 1 and (q.last < q.hw_per or nth == 1024)
        assert plan("split11")[0].last < plan("split11")[0].hw_per


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_forms_select_every_instantiation_and_depth_cases_reach_every_loop_class(dtype, bwd):
    seen = set()
    for form in M.FORMS:
        inst = M.colreduce_instance(dtype, bwd, form)
        seen.add(inst)
        launches, labels = M.depth_case(dtype, bwd, form)
        assert labels >= M.depth_labels_wanted(inst[0]), (form, labels)
        assert all(1 <= len(l) <= 4 for l in launches)
    want = {("bf16", False): {(4, 256, True), (8, 256, True), (4, 1024, True), (4, 256, False), (8, 256, False),
                              (16, 256, False), (4, 1024, False), (8, 1024, False)},
            ("bf16", True): {(4, 256, False), (8, 256, False), (16, 256, False), (4, 1024, False), (8, 1024, False)},
            ("f32", False): {(4, 256, False), (8, 256, False), (4, 1024, False)},
            ("f32", True): {(4, 256, False), (8, 256, False), (4, 1024, False)}}[dtype, bwd]
    assert seen == want


def test_plan_agrees_with_the_library_scratch():
    """gm_spatial_reduce_scratch (host only) = sum of B S C 4 over the problems with S > 1: every NHWC
    case, the two- and four-problem ones included, under 256 and 1024 threads."""
    from greedy_multimodal_learning_amd import _lib as L
    lib = L.load()
    checked = 0
    try:
        for form in M.FORMS:
            L.check(lib.gm_mmtm_set_reduce_form(*form), "form")
            for dtype in DTYPES:
                es = M.ES[dtype]
                cases = [M.col_problems(n, dtype) for n in M.COL_CASES]
                for bwd in (False, True):
                    cases += [(M.DEPTH_B, l) for l in M.depth_case(dtype, bwd, form)[0]]
                for B, probs in cases:
                    items = [L.SpatialReduce(4096, 0, p["C"], p["HW"], 8192, p["C"], 0, 0, 1.0) for p in probs]
                    got = lib.gm_spatial_reduce_scratch(L.arr(L.SpatialReduce, items), len(items), B,
                                                        L.GM_BF16 if dtype == "bf16" else L.GM_F32, L.GM_NHWC)
                    want = sum(M.nhwc_plan(p["C"], p["HW"], B, es, abs(form[0])).scratch for p in probs)
                    assert got == want, (form, dtype, B, probs, got, want)
                    checked += 1
    finally:
        L.check(lib.gm_mmtm_set_reduce_form(*M.DEFAULT_FORM), "form")
    assert checked > 100


def test_row_cases_reach_every_width_and_a_third_trip():
    seen = set()
    for name, (dtype, B, probs, _, trips) in M.ROW_CASES.items():
        for bwd in (False, True):
            vb = M.row_case_width(name, bwd)
            assert vb == M.row_case_wanted(name, bwd), name
            seen.add((dtype, vb, "base" if any("x_off" in p or "dy_off" in p for p in probs) else "hw"))
            assert M.row_trips(probs[0]["HW"], M.ES[dtype], vb) == trips or isinstance(M.ROW_CASES[name][3], tuple)
        assert B * sum(p["C"] for p in probs) > 4                    # more than one workgroup of four waves
    by = lambda how, dtype: {w for d, w, h in seen if (d, h) == (dtype, how)}  # noqa: E731
    assert by("hw", "bf16") >= {16, 8, 4, 2} and by("hw", "f32") >= {16, 8, 4}
    assert by("base", "bf16") >= {8, 4, 2} and by("base", "f32") >= {8, 4}      # a misaligned base lowers the width
    assert any(t == 3 and M.row_case_wanted(n, True) == M.ES[d] for n, (d, _, _, _, t) in M.ROW_CASES.items())
    assert {len(c[2]) for c in M.ROW_CASES.values()} >= {1, 2, 3, 4}


def test_scale_cases_reach_every_form():
    seen = set()
    for name, (layout, B, probs) in M.SCALE_CASES.items():
        for dtype in DTYPES:
            for add in (False, True):
                want = M.SCALE_FORM[name]
                want = want if isinstance(want, str) else want[dtype, add]
                n, form = M.scale_case_form(name, dtype, add)
                assert form == want and n == (1 if form == "one" else 16 // M.ES[dtype]), (name, dtype, add)
                seen.add((dtype, layout, form))
    for dtype in DTYPES:
        assert {f for d, l, f in seen if (d, l) == (dtype, M.NCHW)} == {"vec", "one", "lookup"}
        assert {f for d, l, f in seen if (d, l) == (dtype, M.NHWC)} == {"vec", "one"}
    assert {len(c[2]) for c in M.SCALE_CASES.values()} >= {1, 3, 4}


# ---- the exact tier is exact, and its mutants show -------------------------------------------------------

def _reduce_cases():
    for name, (dtype, B, probs, _, _) in M.ROW_CASES.items():
        yield "row/" + name, dtype, M.NCHW, B, probs
    for name in M.COL_CASES:
        for dtype in DTYPES:
            yield f"col/{name}/{dtype}", dtype, M.NHWC, *M.col_problems(name, dtype)
    done = set()
    for dtype in DTYPES:
        for bwd in (False, True):
            for form in M.FORMS:
                for probs in M.depth_case(dtype, bwd, form)[0]:
                    key = (dtype, tuple(p["HW"] for p in probs))
                    if key not in done:
                        done.add(key)
                        yield f"depth/{dtype}/{key[1]}", dtype, M.NHWC, M.DEPTH_B, probs


REDUCE_MUTANTS = ("drop_last", "no_scale", "e_plain")


def test_reduce_cases_are_exact_and_mutants_change_them(capsys):
    shows = {}
    lines = []
    for label, dtype, layout, B, probs in _reduce_cases():
        for bwd in (False, True):
            rates = {}
            for p, o in zip(probs, M.reduce_case_operands(B, probs)):
                assert bool((o.x != 0).all()) and bool((o.dy != 0).all()) and int(o.x.abs().max()) <= 3
                e0 = p.get("e0", False)
                ref = M.reduce_expected(o, bwd, e0)
                # against integer arithmetic: out * 256 / scale = S k (16 - k)
                s = M.reduce_sum(o, bwd)
                k = o.k[:1] if e0 else o.k
                num = s * k * (16 - k) if bwd else s * 256
                assert int(num.abs().max()) < 2 ** 53 and int(s.abs().max()) * 64 < X.LIMIT
                assert torch.equal(ref * 256 / M.RED_SCALE, num.double())
                assert torch.equal(ref.float().double(), ref)                 # and an fp32 number
                for mut, v in M.reduce_mutants(o, bwd, e0, layout, M.ES[dtype]).items():
                    rates.setdefault(mut, []).append((M.frac_ne(v, ref), ref.numel()))
            for mut, rs in rates.items():
                r = sum(f * n for f, n in rs) / sum(n for _, n in rs)
                assert r >= M.FLOOR, f"{label} bwd={bwd}: {mut} changes only {r:.4f}"
                shows[mut, dtype, layout] = True
                rates[mut] = r
            if not label.startswith("depth"):
                lines.append(f"  reduce {label} {'bwd' if bwd else 'fwd'}: {M.fmt(rates)}")
    for mut in REDUCE_MUTANTS:
        for dtype in DTYPES:
            for layout in (M.NCHW, M.NHWC):
                assert shows.get((mut, dtype, layout)), (mut, dtype, layout)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("name", list(M.SCALE_CASES))
def test_scale_cases_are_exact_inexact_in_bf16_tied_and_mutants_change_them(name, capsys):
    layout, B, probs = M.SCALE_CASES[name]
    for add in (False, True):
        refs = []
        for p, o in zip(probs, M.scale_case_operands(name)):
            assert torch.equal(X.rne(o.x.float()).double(), o.x)              # x is a bf16 number
            assert bool((o.j >= 0).all()) and bool((o.j[:, torch.arange(o.C) % 4 != 1] <= 1024).all())
            ref = M.scale_expected(o, add, p.get("s0", False))
            # against rational arithmetic on the operands, a sample; the integer numerator, everywhere
            for idx in [(0, 0, 0), (B - 1, o.C - 1, o.HW - 1), (B // 2, 1 % o.C, o.HW // 2)]:
                b, c, h = idx
                bs = 0 if p.get("s0") else b
                want = Fraction(int(o.m[b, c, h]), 16) * Fraction(int(o.j[bs, c]), 1024)
                if add:
                    want += Fraction(1, 4) * Fraction(int(o.n[b, c]), 8)
                assert Fraction(float(ref[idx])) == want
            assert torch.equal(ref.float().double(), ref)
            refs.append(ref)
        for dtype in DTYPES:
            want = M.cat(M.scale_case_expected(name, dtype, add))
            rates = {}
            if dtype == "bf16":
                cen = X.bf16_census(M.cat(refs))
                assert cen["inexact"] >= 0.25 and cen["ties"] >= 0.01, (name, add, cen)
                rates.update(inexact=cen["inexact"], ties=cen["ties"])
            muts = {}
            for o, p in zip(M.scale_case_operands(name), probs):
                for mut, v in M.scale_mutants(o, add, p.get("s0", False), dtype).items():
                    muts.setdefault(mut, []).append(v)
            for mut, vs in muts.items():
                rates[mut] = M.frac_ne(M.cat(vs), want)
                assert rates[mut] >= M.FLOOR, f"{name} {dtype} add={add}: {mut} changes only {rates[mut]:.4f}"
            assert set(muts) == ({"trunc", "half_away"} if dtype == "bf16" else set()) | ({"no_alpha"} if add else set())
            with capsys.disabled():
                print(f"\n  scale {name} {dtype} add={int(add)}: {M.fmt(rates)}", end="")


def _gated_expected(name, dtype, flags):
    kind, dt, layout, B, probs, mods = M.gated_problems(name, dtype)
    if kind == "scale":
        return M.cat(M.scale_case_expected(M.GATED_CASES[name][1], dtype, True, flags))
    return M.cat(M.reduce_case_expected(B, probs, True, flags))


def test_gate_mutants_change_the_expected_result_or_are_listed(capsys):
    lines, shows = [], set()
    for name, (kind, base, entry, mods) in M.GATED_CASES.items():
        for dtype in (DTYPES if kind != "row" else [M.ROW_CASES[base][0]]):
            layout = M.gated_problems(name, dtype)[2]
            for label, cur, caring in M.gated_states(name):
                flags = M.substituted(cur, caring, mods)
                want = _gated_expected(name, dtype, flags)
                for mut in M.GATE_MUTANTS[kind]:
                    r = M.frac_ne(_gated_expected(name, dtype, M.gate_mutant_flags(flags)[mut]), want)
                    if (name, label, mut) in M.NOT_CHECKED:
                        assert r == 0.0                                       # listed because it cannot show
                        continue
                    assert r >= M.FLOOR, f"{name} {dtype} {label}: {mut} changes only {r:.4f}"
                    shows.add((mut, dtype, layout))
                    lines.append(f"  gate {name} {dtype} {label}: {mut} {r:.3f}")
    for mut, layouts in (("no_subst", (M.NCHW, M.NHWC)), ("subst_shift", (M.NCHW, M.NHWC)),
                         ("zero_wrong", (M.NCHW, M.NHWC))):
        for layout in layouts:
            assert any((mut, d, layout) in shows for d in DTYPES), (mut, layout)
    assert all((mut, d, M.NHWC) in shows for mut in ("no_subst", "subst_shift", "zero_wrong") for d in DTYPES)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print("  NOT_CHECKED (%d):" % len(M.NOT_CHECKED))
        for (name, label, mut), why in M.NOT_CHECKED.items():
            print(f"    {name} {label} {mut}: {why}")


def test_gate_rule_and_not_checked_name_real_cases():
    assert M.substituted(0, 1, M.MODS2) == [False] * 4 and M.substituted(1, -1, M.MODS2) == [False] * 4
    assert M.substituted(1, 1, M.MODS2) == [False, True, False, False]
    assert M.substituted(1, 2, M.MODS_N["with"]) == [True, False, False, True]
    assert M.substituted(1, 2, M.MODS_N["without"]) == [False] * 4
    for (name, label, mut), why in M.NOT_CHECKED.items():
        assert name in M.GATED_CASES and label in [s[0] for s in M.gated_states(name)] and why
        assert mut in M.GATE_MUTANTS[M.GATED_CASES[name][0]]
    # every gated case is checked in at least one state
    for name, (kind, _, _, mods) in M.GATED_CASES.items():
        live = [s for s in M.gated_states(name) if (name, s[0], M.GATE_MUTANTS[kind][0]) not in M.NOT_CHECKED]
        assert live, name


# ---- the bounded tier -----------------------------------------------------------------------------------------

BOUNDED_REDUCE = [(3, 24, 300), (2, 128, 49)]
BOUNDED_SCALE = [(3, 24, 49)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_bounded_reduce_reference_is_inside_its_own_bound(dtype, bwd, capsys):
    for B, C, HW in BOUNDED_REDUCE:
        c = M.reduce_bounded(B, C, HW, dtype, bwd, M.seed_of("rb", B, C, HW))
        fr = {("rev" if rev else "fwd"): M.used((M.reduce_fp32_emulation(c, rev) - c.ref).abs(), c.bound)
              for rev in (False, True)}
        assert max(fr.values()) <= 1.0, fr
        # a dropped pixel and a missing scale leave the bound
        drop = c.ref - c.scale * (c.x[:, :, -1].double() * (c.dy[:, :, -1].double() if bwd else 1)) * (
            c.e.double() * (1 - c.e.double()) if bwd else 1)
        assert M.violation_rate((drop - c.ref).abs(), c.bound) >= 0.9
        assert M.violation_rate((c.ref / c.scale - c.ref).abs(), c.bound) >= 0.9
        with capsys.disabled():
            print(f"\n  bounded reduce {dtype} {'bwd' if bwd else 'fwd'} {B}x{C}x{HW}: fp32 sums use {M.fmt(fr)}", end="")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
def test_bounded_scale_reference_is_inside_its_own_bound(dtype, add, capsys):
    for B, C, HW in BOUNDED_SCALE:
        c = M.scale_bounded(B, C, HW, dtype, add, M.seed_of("sb", B, C, HW))
        xs = (c.x * c.s[:, :, None]).float()
        y = (xs + ((c.a * torch.tensor(c.alpha, dtype=torch.float32))[:, :, None] if add else 0)).float()
        y = y.to(M.DT[dtype]).double()
        fr = M.used((y - c.ref).abs(), c.bound)
        assert fr <= 1.0
        if dtype == "bf16":      # the store mutants leave the bounded tier too
            assert M.violation_rate((X.trunc(c.ref.float()).double() - c.ref).abs(), c.bound) >= 0.25
        with capsys.disabled():
            print(f"\n  bounded scale {dtype} add={int(add)}: unfused fp32 uses {fr:.3f}", end="")


# ---- running averages -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,step", M.RA_EXACT)
def test_running_average_exact_cases_are_exact(B, step):
    assert B & (B - 1) == 0 and (step + 1) & step == 0
    for C in (1, 65):
        o = M.ra_operands(B, C, C + 3, M.seed_of("ra", B, C, step), exact=True)
        assert bool(torch.isnan(o.e[:, C:]).all())
        nv, ns = M.ra_expected(o, step)
        for c in (0, C - 1):
            m = sum(Fraction(float(o.e[b, c])) for b in range(B)) / B
            assert Fraction(float(nv[c])) == (m + Fraction(float(o.rv[c])) * step) / (step + 1)
            assert Fraction(float(ns[c])) == (m + Fraction(float(o.rs[c])) * step) / (step + 1)
        ev, es = M.ra_fp32_emulation(o, step)
        assert torch.equal(ev, nv) and torch.equal(es, ns)      # every fp32 intermediate is exact
        assert torch.equal(nv.float().double(), nv)


@pytest.mark.parametrize("B,step", M.RA_BOUNDED)
def test_running_average_bound_holds_the_emulation_and_rejects_the_mutants(B, step, capsys):
    C = 257
    o = M.ra_operands(B, C, C, M.seed_of("ra", B, C, step), exact=False)
    nv, ns = M.ra_expected(o, step)
    bv, bs = M.ra_bound(o)
    ev, es = M.ra_fp32_emulation(o, step)
    fr = max(M.used((ev - nv).abs(), bv), M.used((es - ns).abs(), bs))
    assert fr <= 1.0
    _, own = M.ra_expected(o, step, own_mean=True)
    dv, _ = M.ra_expected(o, step, div_step=True)
    rates = dict(own_mean=M.violation_rate((own - ns).abs(), bs), div_step=M.violation_rate((dv - nv).abs(), bv))
    for k, r in rates.items():
        assert r >= M.FLOOR, (k, r)
    with capsys.disabled():
        print(f"\n  running avg B={B} step={step}: emulation uses {fr:.3f}; mutants violate {M.fmt(rates)}", end="")
