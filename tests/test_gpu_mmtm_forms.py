"""The MMTM site kernels (csrc/mmtm_kernels.hip) and the gate's MMTM kernels (csrc/gate.hip) per
form, against the rules and references of mmtmref.py (whose conditions test_cpu_mmtmref.py proves).

Exact tier: operands on which every fp32 intermediate is exact in any order, so each output must be
torch.equal to the fp64 value, rounded once where it is stored as bf16.  Covered: every vector width
of k_rowreduce_nchw (through HW and through a misaligned base), forward and backward; every
instantiation of k_colreduce_nhwc the eight forms select, both dtypes, at pixel counts that give a
thread 0, 1-3, exactly U, U + 4 + a tail and 2U + a tail pixels, with splits, idle lanes, one and two
channel slabs, and launches that mix S > 1 with S == 1; the vector, one-element and per-element
lookup forms of k_channel_scale; the gated entry points under a real gm_gate_state and a
gm_gate_state_n in every state; gm_mmtm_select_scale, gm_mmtm_mask_rows, gm_mmtm_mask_rows2; the two
running-average entry points, which must also equal each other bit for bit.  One bounded-tier row
per kernel family prints the fraction of its derived bound the device uses.  Outputs are pre-filled
with NaN: an unwritten element fails."""
import contextlib
import ctypes

import pytest
import torch

import mmtmref as M

pytestmark = pytest.mark.gpu
DTYPES = ["bf16", "f32"]
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def lib_mod():
    from greedy_multimodal_learning_amd import _lib
    return _lib


def ops_mod():
    from greedy_multimodal_learning_amd import ops
    return ops


def consts(dtype, layout):
    L = lib_mod()
    return (L.GM_BF16 if dtype == "bf16" else L.GM_F32), (L.GM_NHWC if layout == M.NHWC else L.GM_NCHW)


def place(t, dtype, layout, dev, off=0):
    """[B, C, HW] values -> a flat device tensor in the layout's order, `off` elements into its buffer."""
    t = t.to(dev)
    flat = (t.permute(0, 2, 1) if layout == M.NHWC else t).contiguous().reshape(-1).to(M.DT[dtype])
    if not off:
        return flat
    buf = torch.zeros(flat.numel() + off + 16, dtype=M.DT[dtype], device=dev)
    view = buf[off:off + flat.numel()]
    view.copy_(flat)
    return view


def unplace(y, B, C, HW, layout):
    y = y.float().cpu()
    return y.view(B, HW, C).permute(0, 2, 1) if layout == M.NHWC else y.view(B, C, HW)


def rows(vals, ld, off, dev):
    """[B, C] values as rows of stride ld starting `off` floats into a NaN-filled buffer."""
    B, C = vals.shape
    buf = torch.full((off + B * ld + 4,), NAN)
    buf[off:off + B * ld].view(B, ld)[:, :C] = vals.float()
    return buf.to(dev)


@contextlib.contextmanager
def reduce_form(form):
    L = lib_mod()
    try:
        L.check(L.load().gm_mmtm_set_reduce_form(*form), "form")
        yield
    finally:
        L.check(L.load().gm_mmtm_set_reduce_form(*M.DEFAULT_FORM), "form")


def gate_state(dev, kind, cur, caring):
    """A gm_gate_state ("state") or gm_gate_state_n ("state_n") in device memory; everything past the
    curation_mode / caring prefix holds values a wrong offset would trip over."""
    L = lib_mod()
    if kind == "state":
        st = L.GateState(cur, caring, 3, 1, 7, 9, 0x5A5A5A5A, 0x5A5A5A5A, 0.01, (ctypes.c_double * 4)(1, 2, 3, 4), 0.5)
    else:
        st = L.GateStateN()
        st.curation_mode, st.caring, st.curation_step, st.unlock = cur, caring, 3, 1
        st.window, st.n_curated, st.nb, st.pad0, st.eps, st.d_bdr = 7, 9, 4, 0x5A5A5A5A, 0.01, 0.5
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(dev)


# ---- squeeze and squeeze backward -------------------------------------------------------------------------------

def run_reduce(dev, dtype, layout, B, probs, bwd, gate=None, mods=None, poison=None):
    """One launch; returns the [B, C] outputs per problem (fp64, CPU).  poison: problem index whose dy
    gets an inf and a NaN."""
    dt, lay = consts(dtype, layout)
    launch, outs = [], []
    for i, (p, o) in enumerate(zip(probs, M.reduce_case_operands(B, probs))):
        C, HW = p["C"], p["HW"]
        pad = (C + HW + i) % 2 * 5                          # ld_out > C with an output offset on some
        out = torch.full((B, C + pad), NAN, device=dev)
        d = dict(x=place(o.x, dtype, layout, dev, p.get("x_off", 0)), C=C, HW=HW, out=out, ld_out=C + pad,
                 out_off=pad // 2, scale=M.RED_SCALE)
        if bwd:
            dy = o.dy.float()
            if poison == i:
                dy = dy.clone()
                dy[0, 0, HW // 2] = float("inf")
                dy[B - 1, C - 1, HW - 1] = NAN
            d.update(dy=place(dy, dtype, layout, dev, p.get("dy_off", 0)), e=(o.k.float() / 16).to(dev),
                     ld_e=0 if p.get("e0") else C)
        launch.append(d)
        outs.append((out, pad // 2, C, pad))
    ops_mod().spatial_reduce(launch, B, dt, lay, dev, gate=gate, mods=mods)
    res = []
    for out, off, C, pad in outs:
        o = out.cpu().double()
        keep = torch.ones(C + pad, dtype=torch.bool)
        keep[off:off + C] = False
        assert bool(torch.isnan(o[:, keep]).all()), "wrote outside its C columns"
        res.append(o[:, off:off + C])
    return res


def assert_reduce(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g.float(), w.float()), f"{what} problem {i}: {M.frac_ne(g, w):.4f} of the outputs differ"


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("name", list(M.ROW_CASES))
def test_rowreduce_exact(dev, name, bwd):
    dtype, B, probs, _, _ = M.ROW_CASES[name]
    assert M.row_case_width(name, bwd) == M.row_case_wanted(name, bwd)
    got = run_reduce(dev, dtype, M.NCHW, B, probs, bwd)
    assert_reduce(got, M.reduce_case_expected(B, probs, bwd), name)


@pytest.mark.parametrize("form", M.FORMS, ids=[f"{t}x{u}" for t, u in M.FORMS])
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_colreduce_exact_under_every_form(dev, dtype, bwd, form):
    launches, labels = M.depth_case(dtype, bwd, form)
    assert labels >= M.depth_labels_wanted(M.colreduce_instance(dtype, bwd, form)[0])
    with reduce_form(form):
        for name in M.COL_CASES:
            B, probs = M.col_problems(name, dtype)
            got = run_reduce(dev, dtype, M.NHWC, B, probs, bwd)
            assert_reduce(got, M.reduce_case_expected(B, probs, bwd), f"{name} {form}")
        for probs in launches:
            got = run_reduce(dev, dtype, M.NHWC, M.DEPTH_B, probs, bwd)
            assert_reduce(got, M.reduce_case_expected(M.DEPTH_B, probs, bwd), f"depth {[p['HW'] for p in probs]} {form}")


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("layout", [M.NCHW, M.NHWC])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_bounded(dev, dtype, layout, bwd, capsys):
    """N(0, 1) operands, scale = 1 / HW: inside gamma_{HW+3} |scale| |e (1 - e)| sum |t_i| of fp64."""
    dt, lay = consts(dtype, layout)
    fr = {}
    for B, C, HW in [(3, 24, 300), (2, 128, 49)]:
        c = M.reduce_bounded(B, C, HW, dtype, bwd, M.seed_of("rb", B, C, HW))
        out = torch.full((B, C), NAN, device=dev)
        d = dict(x=place(c.x, dtype, layout, dev), C=C, HW=HW, out=out, ld_out=C, scale=c.scale)
        if bwd:
            d.update(dy=place(c.dy, dtype, layout, dev), e=c.e.to(dev), ld_e=C)
        ops_mod().spatial_reduce([d], B, dt, lay, dev)
        fr[f"{B}x{C}x{HW}"] = M.used((out.cpu().double() - c.ref).abs(), c.bound)
    with capsys.disabled():
        print(f"\n  bounded reduce {dtype} {layout} {'bwd' if bwd else 'fwd'}: used {M.fmt(fr)}", end="")
    assert max(fr.values()) <= 1.0, fr


# ---- channel scale --------------------------------------------------------------------------------------------------

def run_scale(dev, name, dtype, add, gate=None, mods=None, gated=False):
    """One launch of a SCALE_CASES case; returns y per problem as [B, C, HW] fp32 on the CPU."""
    layout, B, probs = M.SCALE_CASES[name]
    dt, lay = consts(dtype, layout)
    launch, ys, alts = [], [], []
    for p, o in zip(probs, M.scale_case_operands(name)):
        C, HW = p["C"], p["HW"]
        y = torch.full((B * C * HW,), NAN, device=dev, dtype=M.DT[dtype])
        ld = C + p.get("pad_s", 0)
        d = dict(x=place(o.x, dtype, layout, dev, p.get("x_off", 0)), y=y, C=C, HW=HW,
                 s=rows(o.s, ld, p.get("s_off", 0), dev), s_off=p.get("s_off", 0), ld_s=0 if p.get("s0") else ld)
        if add:
            d.update(a=rows(o.a, C, p.get("a_off", 0), dev), a_off=p.get("a_off", 0), ld_a=C, alpha=M.ALPHA)
        launch.append(d)
        ys.append((y, C, HW))
        alts.append(o.alt_s.float().to(dev))
    ops_mod().channel_scale(launch, B, dt, lay, dev, gate=gate, alt=alts if gated else None, mods=mods)
    return [unplace(y, B, C, HW, layout) for y, C, HW in ys]


def assert_scale(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f"{what} problem {i}: {M.frac_ne(g, w):.4f} of the outputs differ"


@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(M.SCALE_CASES))
def test_channel_scale_exact(dev, name, dtype, add):
    want_form = M.SCALE_FORM[name]
    assert M.scale_case_form(name, dtype, add)[1] == (want_form if isinstance(want_form, str) else want_form[dtype, add])
    assert_scale(run_scale(dev, name, dtype, add), M.scale_case_expected(name, dtype, add), name)


@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("layout", [M.NCHW, M.NHWC])
@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_scale_bounded(dev, dtype, layout, add, capsys):
    """N(0, 1) x, sigmoid s, alpha = 1 / HW: inside 3 u (|x s| + |alpha a|) + half a bf16 ulp of fp64."""
    dt, lay = consts(dtype, layout)
    B, C, HW = 3, 24, 49
    c = M.scale_bounded(B, C, HW, dtype, add, M.seed_of("sb", B, C, HW))
    y = torch.full((B * C * HW,), NAN, device=dev, dtype=M.DT[dtype])
    d = dict(x=place(c.x, dtype, layout, dev), y=y, C=C, HW=HW, s=c.s.to(dev), ld_s=C)
    if add:
        d.update(a=c.a.to(dev), ld_a=C, alpha=c.alpha)
    ops_mod().channel_scale([d], B, dt, lay, dev)
    fr = M.used((unplace(y, B, C, HW, layout).double() - c.ref).abs(), c.bound)
    with capsys.disabled():
        print(f"\n  bounded scale {dtype} {layout} add={int(add)}: used {fr:.3f}", end="")
    assert fr <= 1.0


# ---- the gated entry points ---------------------------------------------------------------------------------------------

def gated_ids():
    return [(n, d) for n, c in M.GATED_CASES.items() for d in (DTYPES if c[0] != "row" else [M.ROW_CASES[c[1]][0]])]


@pytest.mark.parametrize("kind", ["state", "state_n"])
@pytest.mark.parametrize("name,dtype", [g for g in gated_ids() if M.GATED_CASES[g[0]][0] == "scale"])
def test_channel_scale_gated_by_the_rule(dev, name, dtype, kind):
    """A substituted problem equals the exact reference with s := its alt row broadcast, every other
    the plain reference - in every state, through the two-modality and the N-modality entry point."""
    _, base, entry, mods = M.GATED_CASES[name]
    for add in (False, True):
        for label, cur, caring in M.gated_states(name):
            flags = M.substituted(cur, caring, mods)
            got = run_scale(dev, base, dtype, add, gate=gate_state(dev, kind, cur, caring),
                            mods=mods if entry == "n" else None, gated=True)
            assert_scale(got, M.scale_case_expected(base, dtype, add, flags), f"{name} {label} add={add}")


@pytest.mark.parametrize("kind", ["state", "state_n"])
@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("name,dtype", [g for g in gated_ids() if M.GATED_CASES[g[0]][0] != "scale"])
def test_spatial_reduce_gated_by_the_rule(dev, name, dtype, bwd, kind):
    """A substituted problem's outputs are 0, every other equals the plain reference; NHWC with
    S > 1 applies the factor in k_reduce_partials."""
    _, _, layout, B, probs, mods = M.gated_problems(name, dtype)
    entry = M.GATED_CASES[name][2]
    if layout == M.NHWC:
        assert any(M.nhwc_plan(p["C"], p["HW"], B, M.ES[dtype]).S > 1 for p in probs)
    for label, cur, caring in M.gated_states(name):
        flags = M.substituted(cur, caring, mods)
        got = run_reduce(dev, dtype, layout, B, probs, bwd, gate=gate_state(dev, kind, cur, caring),
                         mods=mods if entry == "n" else None)
        assert_reduce(got, M.reduce_case_expected(B, probs, bwd, flags), f"{name} {label}")


@pytest.mark.parametrize("name,dtype", [("row-2prob", "bf16"), ("col-mixedS", "bf16"), ("col-mixedS", "f32")])
def test_spatial_reduce_gated_keeps_nan_as_mask_rows2_does(dev, name, dtype):
    """The gated form multiplies by 0, so a non-finite gradient in the substituted modality stays
    NaN: the output is what gm_mmtm_mask_rows2 makes of the ungated output."""
    L = lib_mod()
    _, _, layout, B, probs, mods = M.gated_problems(name, dtype)
    for caring in (0, 1):
        plain = run_reduce(dev, dtype, layout, B, probs, True, poison=caring)
        assert int((~torch.isfinite(plain[caring])).sum()) == 2
        got = run_reduce(dev, dtype, layout, B, probs, True, gate=gate_state(dev, "state", 1, caring), poison=caring)
        a, b = (t.float().contiguous().to(dev) for t in plain)
        mask = torch.tensor([0.0 if caring == 0 else 1.0, 0.0 if caring == 1 else 1.0], device=dev)
        L.check(L.load().gm_mmtm_mask_rows2(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), mask.data_ptr(),
                                            L.stream_of(dev)), "gm_mmtm_mask_rows2")
        for g, w, p in zip(got, (a.cpu(), b.cpu()), plain):
            assert M.same(g, w)
        sub = got[caring]
        assert torch.equal(torch.isnan(sub), ~torch.isfinite(plain[caring])) and bool((sub[~torch.isnan(sub)] == 0).all())
        assert torch.equal(got[1 - caring], plain[1 - caring])


# ---- gm_mmtm_select_scale, gm_mmtm_mask_rows, gm_mmtm_mask_rows2 ----------------------------------------------------------

GRID_CAP = 1024 * 256      # the three kernels' grids stop at 1024 workgroups of 256 threads


@pytest.mark.parametrize("kind", ["state", "state_n"])
@pytest.mark.parametrize("B,Cv,Cs", [(3, 5, 7), (64, 2047, 2048), (64, 2048, 2049)], ids=["small", "below", "above"])
def test_select_scale_by_the_rule(dev, B, Cv, Cs, kind):
    L = lib_mod()
    assert Cv != Cs and ((B * (Cv + Cs) > GRID_CAP) == (Cv == 2048)) and (B < 64 or abs(B * (Cv + Cs) - GRID_CAP) < 100)
    g = torch.Generator().manual_seed(B + Cv)
    ld_v, ld_s = Cv + 3, Cs
    e_v, e_s = torch.rand(B, Cv, generator=g), torch.rand(B, Cs, generator=g)
    ra_v, ra_s = torch.rand(Cv, generator=g) + 2, torch.rand(Cs, generator=g) + 4      # told apart from e by range
    EV = rows(e_v, ld_v, 0, dev)
    ES, RV, RS = e_s.to(dev), ra_v.to(dev), ra_s.to(dev)
    for label, cur, caring in M.GATE_STATES_N:
        s_v, s_s = torch.full((B, Cv), NAN, device=dev), torch.full((B, Cs), NAN, device=dev)
        mask = torch.full((2,), NAN, device=dev)
        L.check(L.load().gm_mmtm_select_scale(EV.data_ptr(), ld_v, ES.data_ptr(), ld_s, RV.data_ptr(), RS.data_ptr(),
                                              B, Cv, Cs, gate_state(dev, kind, cur, caring).data_ptr(), s_v.data_ptr(),
                                              s_s.data_ptr(), mask.data_ptr(), L.stream_of(dev)), "gm_mmtm_select_scale")
        wv, ws, wm = M.select_scale_rule(e_v, e_s, ra_v, ra_s, cur, caring)
        assert torch.equal(s_v.cpu(), wv) and torch.equal(s_s.cpu(), ws), label
        m = mask.cpu()
        assert torch.equal(m, wm) and set(m.tolist()) <= {0.0, 1.0}, label


@pytest.mark.parametrize("n", [5, GRID_CAP - 7, GRID_CAP + 257], ids=["small", "below", "above"])
def test_mask_rows_by_the_rule(dev, n):
    L = lib_mod()
    g = torch.Generator().manual_seed(n)
    a0 = torch.randint(-9, 10, (n + 1,), generator=g).float()
    a0[n // 2], a0[n] = float("inf"), 77.0                           # a[n] lies past the range
    for k in (0.0, 1.0):
        a = a0.to(dev)
        mask = torch.tensor([k, NAN], device=dev)
        L.check(L.load().gm_mmtm_mask_rows(a.data_ptr(), n, mask.data_ptr(), L.stream_of(dev)), "gm_mmtm_mask_rows")
        want = a0 * k
        want[n] = 77.0
        assert M.same(a.cpu(), want) and bool(torch.isnan(want[n // 2]) == (k == 0.0))


@pytest.mark.parametrize("na,nb", [(5, 9), (GRID_CAP - 300, 200), (300, GRID_CAP - 200), (GRID_CAP // 2 + 1, GRID_CAP)],
                         ids=["small", "below", "above", "twice"])
def test_mask_rows2_by_the_rule(dev, na, nb):
    L = lib_mod()
    assert na != nb
    g = torch.Generator().manual_seed(na + nb)
    a0, b0 = (torch.randint(1, 10, (n + 1,), generator=g).float() for n in (na, nb))     # nonzero; [n] past the range
    for ka, kb in ((0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.0, 0.0)):
        a, b = a0.to(dev), b0.to(dev)
        mask = torch.tensor([ka, kb], device=dev)
        L.check(L.load().gm_mmtm_mask_rows2(a.data_ptr(), na, b.data_ptr(), nb, mask.data_ptr(), L.stream_of(dev)),
                "gm_mmtm_mask_rows2")
        wa, wb = a0 * ka, b0 * kb
        wa[na], wb[nb] = a0[na], b0[nb]
        ga, gb = a.cpu(), b.cpu()
        assert torch.equal(ga, wa) and torch.equal(gb, wb)
        # the boundary element of each range
        assert float(ga[na - 1]) == float(a0[na - 1]) * ka and float(gb[0]) == float(b0[0]) * kb
        assert float(gb[nb - 1]) == float(b0[nb - 1]) * kb and float(ga[na]) == float(a0[na])


# ---- running averages ---------------------------------------------------------------------------------------------------------

def run_ra(dev, o, step, increment=1):
    """Both entry points on one case: (new_v, new_s) of gm_mmtm_running_avg, (ra_v, ra_s) of
    gm_mmtm_running_avg_dev after the in-place update, and the device counter after it."""
    ops = ops_mod()
    E = o.e.to(dev)[:, :o.C]                               # a view: ld_e = the buffer's row stride
    assert E.stride(0) == o.e.shape[1]
    nv, ns = ops.running_avg(E, o.rv.to(dev), o.rs.to(dev), step)
    rv, rs = o.rv.to(dev), o.rs.to(dev)
    counter = torch.tensor([step], dtype=torch.int32, device=dev)
    ops.running_avg_dev(E, rv, rs, counter, increment=increment)
    return (nv.cpu(), ns.cpu()), (rv.cpu(), rs.cpu()), int(counter.cpu())


@pytest.mark.parametrize("C", M.RA_C)
def test_running_avg_exact_and_the_two_entry_points_equal(dev, C):
    for B, step in M.RA_EXACT:
        o = M.ra_operands(B, C, C + 3, M.seed_of("ra", B, C, step), exact=True)
        wv, ws = (t.float() for t in M.ra_expected(o, step))
        (nv, ns), (rv, rs), counter = run_ra(dev, o, step)
        assert torch.equal(nv, wv) and torch.equal(ns, ws), (B, step)
        assert torch.equal(rv, wv) and torch.equal(rs, ws), (B, step)
        assert counter == step + 1


@pytest.mark.parametrize("B,step", M.RA_BOUNDED)
def test_running_avg_bounded_and_the_two_entry_points_equal(dev, B, step, capsys):
    """Uniform e: inside gamma_{B+4} (|m| + |ra|) of the fp64 recurrence, and gm_mmtm_running_avg_dev
    bit-equal to gm_mmtm_running_avg (the header: "Same arithmetic") at every C."""
    fr = 0.0
    for C in M.RA_C:
        o = M.ra_operands(B, C, C + 5, M.seed_of("ra", B, C, step), exact=False)
        wv, ws = M.ra_expected(o, step)
        bv, bs = M.ra_bound(o)
        (nv, ns), (rv, rs), _ = run_ra(dev, o, step)
        assert torch.equal(nv, rv) and torch.equal(ns, rs), f"C={C}: the two entry points differ"
        fr = max(fr, M.used((nv.double() - wv).abs(), bv), M.used((ns.double() - ws).abs(), bs))
    with capsys.disabled():
        print(f"\n  bounded running avg B={B} step={step}: used {fr:.3f}", end="")
    assert fr <= 1.0


def test_running_avg_alias_and_device_counter(dev):
    """ra_s aliasing ra_v is updated once; increment = 0 leaves the counter, increment = 1 advances
    it; two back-to-back calls that share one counter value, as MMTM_N issues them."""
    ops = ops_mod()
    B, C, step = 17, 257, 1000
    o = M.ra_operands(B, C, C, M.seed_of("ra-alias"), exact=False)
    E = o.e.to(dev)
    (nv, ns), _, _ = run_ra(dev, o, step)
    # the alias, both entry points
    r = o.rv.to(dev)
    av, as_ = ops.running_avg(E, r, r, step)
    assert torch.equal(av.cpu(), nv) and torch.equal(as_.cpu(), nv)
    counter = torch.tensor([step], dtype=torch.int32, device=dev)
    ops.running_avg_dev(E, r, r, counter, increment=False)
    assert torch.equal(r.cpu(), nv) and int(counter.cpu()) == step
    # two calls on one counter value: the first leaves it, the second advances it once
    ra = [o.rv.to(dev), o.rs.to(dev), o.rv.to(dev)]
    ops.running_avg_dev(E, ra[0], ra[1], counter, increment=False)
    ops.running_avg_dev(E, ra[2], ra[2], counter, increment=True)
    assert int(counter.cpu()) == step + 1
    assert torch.equal(ra[0].cpu(), nv) and torch.equal(ra[1].cpu(), ns) and torch.equal(ra[2].cpu(), nv)
    # and the exact tier through the alias: a second update would show
    o = M.ra_operands(16, 65, 65, M.seed_of("ra-alias-exact"), exact=True)
    r = o.rv.to(dev)
    counter = torch.tensor([7], dtype=torch.int32, device=dev)
    ops.running_avg_dev(o.e.to(dev), r, r, counter)
    assert torch.equal(r.cpu(), M.ra_expected(o, 7)[0].float()) and int(counter.cpu()) == 8
