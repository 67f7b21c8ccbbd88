"""The BatchNorm kernels of csrc/bn_act.hip against float64, on every launch form: two launches (float4 / scalar / split over images),
one launch (<4> / <1>, both sides of its 5120-vector limit, groups), the stem's pooled forms (even W: rows kernels; odd W: generic
kernel + in-place apply).  Inputs and the float64 reference come from tests/bn_cases.py; tests/test_bn_cases_host.py holds, on the CPU,
what makes the comparison exact (no pre-activation within 1e-3 of the output scale of the ReLU kink, no pooling window tied).

Two arms per case, each an error against float64 as a fraction of the reference tensor's max-abs:
    e_hip    the HIP kernels (functional.bn_act / functional.bn_relu_maxpool)
    e_torch  nn.BatchNorm2d in fp32 on the device, on the same input (torch / MIOpen: the arithmetic the kernels replace)
Rule, for every quantity:  e_hip <= max(b0 * f, 4 * e_torch).
    b0 is test_gpu_bn.py's bar: 2e-5 for y / dres / the running and saved statistics, 5e-5 for dx, 1e-4 for dgamma / dbeta.
    The margin of 4 over e_torch covers a different but equally valid summation order; e_hip never sets its own bar.
    f = 1 except for the `offset` cases, where f = 1 + kappa / 16, kappa = max |mu| / sigma:
        the apply pass is y = fmaf(x, scale, shift) with shift = beta - mean * scale rounded ONCE to fp32.  |mean * scale| =
        kappa * |gamma| (in units of the output's standard deviation), so that rounding alone moves y by eps32 * kappa * |gamma|,
        eps32 = 6e-8.  Outputs have a max-abs of about 4 |gamma| sigma-units and the mean, rstd and scale that enter the product each
        carry a rounding of their own (a factor of about 4): relative to the output scale the error is ~ 4 * 6e-8 * kappa / 4 ... the
        same order as b0 * kappa / 16 = 1.25e-6 * kappa with b0 = 2e-5 left as the floor for kappa -> 0.  No fp32 kernel that forms
        x * scale + shift can do better, and torch's fp32 BatchNorm (e_torch) is printed beside it.
    first_pixel, flat, tiny_var: f = 1.  The kernels' variance is s2/n - (s1/n)^2 of x - K, whose relative error grows like
        eps32 * (1 + (K - mu)^2 / sigma^2).  With K = x_first (the kernels before this file) that is eps32 * (1 + delta^2), delta =
        |x_first - mu| / sigma, and delta = 64 missed the rule by 25 x; K (bn_shift) is still x_first unless that is an outlier among its 15 neighbours, then their mean.
Elements left out of the element-wise gradient comparison: none for the forward outputs; for dx / dres those whose ReLU decision
differs from float64's, at most 1e-5 of the elements (none at all for the pooled forms).

The BatchNorm entry points are not among those _lib.TIMING brackets (they are called ~270 times per step), so "the entry point ran" is
asserted with a counting shim on the bound library instead."""
import contextlib
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_cases as B  # noqa: E402

pytestmark = pytest.mark.gpu

B0 = dict(y=2e-5, dres=2e-5, running_mean=2e-5, running_var=2e-5, save_mean=2e-5, save_rstd=2e-5, dx=5e-5, dgamma=1e-4, dbeta=1e-4)
MARGIN = 4.0
MAX_FLIPS = 1e-5


def _rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-300))


@contextlib.contextmanager
def _counting(*names):
    """Counts the calls of the named entry points (ops fetches them from the bound library at every call)."""
    from shapeclipper_amd import _lib
    lib, calls, saved = _lib.load(), {}, {}

    def shim(name, fn):
        def call(*args):
            calls[name] = calls.get(name, 0) + 1
            return fn(*args)
        return call
    for n in names:
        saved[n] = getattr(lib, n)
        setattr(lib, n, shim(n, saved[n]))
    try:
        yield calls
    finally:
        for n, fn in saved.items():
            setattr(lib, n, fn)


def _module(c):
    bn = nn.BatchNorm2d(c.shape[1], eps=B.EPS, momentum=B.MOMENTUM, track_running_stats=c.track).cuda()
    with torch.no_grad():
        bn.weight.copy_(c.gamma)
        bn.bias.copy_(c.beta)
        if c.track:
            bn.running_mean.copy_(c.rm0)
            bn.running_var.copy_(c.rv0)
    return bn.train(c.training)


def _collect(c, bn, x, res, y, stats):
    y.backward(c.cot.cuda())
    out = dict(y=y.detach(), dx=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, save_mean=stats[0], save_rstd=stats[1])
    if c.with_res:
        out["dres"] = res.grad
    if c.track and c.training:
        out["running_mean"], out["running_var"] = bn.running_mean.clone(), bn.running_var.clone()
        out["num_batches_tracked"] = int(bn.num_batches_tracked)
    return out


def _leaves(c):
    x = c.x.cuda().requires_grad_(True)
    return x, (c.res.cuda().requires_grad_(True) if c.with_res else None)


def _hip(c):
    from shapeclipper_amd.functional import bn_act, bn_relu_maxpool
    bn = _module(c)
    x, res = _leaves(c)
    fwd, bwd = ("sc_bn_relu_pool_forward", "sc_bn_relu_pool_backward") if c.pool else ("sc_bn_act_forward", "sc_bn_act_backward")
    with _counting(fwd, bwd) as calls:
        y = bn_relu_maxpool(bn, x, groups=c.groups) if c.pool else bn_act(bn, x, residual=res, relu=c.relu, groups=c.groups)
        stats = y.grad_fn.saved_tensors[3].clone()                  # [2, G, C]: save_mean, save_rstd
        out = _collect(c, bn, x, res, y, stats)
    assert calls == {fwd: 1, bwd: 1}, calls
    return out


def _torch32(c):
    """nn.BatchNorm2d in fp32 on the device, one call per group in order."""
    bn = _module(c)
    x, res = _leaves(c)
    training = c.training or not c.track
    with torch.no_grad():
        if training:
            st = [torch.native_batch_norm(t, bn.weight, bn.bias, None, None, True, B.MOMENTUM, B.EPS)[1:] for t in x.chunk(c.groups)]
            stats = torch.stack([torch.stack([s[0] for s in st]), torch.stack([s[1] for s in st])])
        else:
            stats = torch.stack([bn.running_mean, (bn.running_var + B.EPS).rsqrt()])[:, None].expand(2, c.groups, -1)
    y = torch.cat([bn(t) for t in x.chunk(c.groups)], 0)
    if res is not None:
        y = y + res
    if c.relu:
        y = torch.relu(y)
    if c.pool:
        y = F.max_pool2d(y, 3, 2, 1)
    return _collect(c, bn, x, res, y, stats)


def _errors(c, got, ref, channels=None):
    """{quantity: error}; dx / dres without the elements whose ReLU decision differs from float64's (their share is returned too)."""
    errs, flips = {}, 0.0
    away = None
    if c.relu and not c.pool:
        differ = (got["y"].cpu() > 0) != (ref["z"] > 0)
        flips = float(differ.sum()) / differ.numel()
        away = ~differ
    for q in B.QUANTITIES:
        if q not in ref:
            continue
        a, b = got[q].double().cpu(), ref[q]
        dim = 1 if a.dim() == 4 else -1
        if channels is not None:
            a, b = a.index_select(dim, channels), b.index_select(dim, channels)
        d = (a - b).abs()
        if q in ("dx", "dres") and away is not None:
            d = d * (away if channels is None else away.index_select(1, channels))
        errs[q] = float(d.max() / b.abs().max().clamp_min(1e-300))
    return errs, flips


def _judge(c, what, f=1.0, channels=None, hip=None, t32=None):
    ref = B.reference(c)
    hip = _hip(c) if hip is None else hip
    t32 = _torch32(c) if t32 is None else t32
    eh, flips = _errors(c, hip, ref, channels)
    et, _ = _errors(c, t32, ref, channels)
    bad = []
    for q, e in eh.items():
        bar = max(B0[q] * f, MARGIN * et[q])
        print("BN64 | %s | %s | e_hip %.3e | e_torch %.3e | bar %.3e" % (what, q, e, et[q], bar))
        if not e <= bar:
            bad.append("%s: e_hip %.3e > bar %.3e (e_torch %.3e)" % (q, e, bar, et[q]))
    if "num_batches_tracked" in hip:
        assert hip["num_batches_tracked"] == t32["num_batches_tracked"] == c.groups
    print("BN64 | %s | relu flips | %.3e of the elements" % (what, flips))
    assert flips <= MAX_FLIPS, "%s: %.3e of the elements change side of the ReLU" % (what, flips)
    assert not bad, "%s: %s" % (what, "; ".join(bad))


VARIANTS = [(True, False, True, True), (True, True, True, True), (False, False, True, True), (False, True, True, True),
            (True, False, False, True), (True, True, False, True), (False, False, False, True), (False, True, False, True),
            (True, True, True, False)]          # relu, with_res, training, track_running_stats
STEM_VARIANTS = [(True, False, True, True), (True, False, False, True), (True, False, True, False)]       # the stem form is relu(bn(x)) only
ROW_CASES = [(row, v) for row in B.ROWS for v in (STEM_VARIANTS if row[3] else VARIANTS)]


@pytest.mark.parametrize("row,variant", ROW_CASES, ids=["%s-%s-g%d-relu%d-res%d-train%d-track%d" % ((r[0], "x".join(map(str, r[1])), r[2]) + v)
                                                        for r, v in ROW_CASES])
def test_every_launch_form_against_float64(row, variant):
    form, shape, groups, pool = row
    relu, with_res, training, track = variant
    c = B.make(shape, groups, relu=relu, with_res=with_res, training=training, pool=pool, track=track)
    _judge(c, "%s %s g%d relu%d res%d train%d track%d" % (form, shape, groups, relu, with_res, training, track))


@pytest.mark.parametrize("pair", B.BOUNDARY_PAIRS, ids=["float4", "scalar"])
def test_both_sides_of_the_one_launch_limit_meet_the_same_bar(pair):
    """5096 vectors take the one-launch kernel, 5145 the two-launch pair: nothing at the Python level names the choice, so both
    neighbours are held to the same float64 bar (a limit off by one image would run a kernel on a shape it cannot hold)."""
    for shape in pair:
        assert B.fused_takes(shape[0], shape[1], shape[2] * shape[3], 1) == (shape[0] == 104)
        _judge(B.make(shape, 1, relu=True, with_res=True, training=True), "limit %s" % (shape,))


COND_CASES = [(n, kind, k, d, shape, pool) for n, kind, k, d in B.COND for shape, pool in B.COND_SHAPES] + \
             [("first_pixel_64", "first_pixel", 0.3, 64.0, shape, pool) for shape, pool in B.FIRST_PIXEL_64]


@pytest.mark.parametrize("name,kind,kappa,delta,shape,pool", COND_CASES, ids=["%s-%s" % (c[0], "x".join(map(str, c[4]))) for c in COND_CASES])
def test_conditioning_cases_against_float64(name, kind, kappa, delta, shape, pool):
    """first_pixel_64 (at 20x16x16x16, 80x256x8x8 and 2x4x52x52: delta <= sqrt(n - 1)) is the case that made the variance shift robust:
    with K = x_first 64 sigma from the mean, s2/n - (s1/n)^2 lost eps32 * (1 + 64^2) = 2.4e-4 of the variance -- save_rstd 4.0e-4 /
    5.3e-4 / 5.0e-4, y 3.6e-4 / 5.1e-4 / 8.7e-5, dx 4.1e-4 / 2.5e-4 / 2.4e-4 of max against e_torch <= 3.3e-7.  bn_shift now replaces an
    x_first that is more than 8 x the spread of its 15 neighbours away from their mean by that mean.  docs/LAB_NOTEBOOK.md section 17."""
    c = B.make(shape, 1, kind=kind, kappa=kappa, delta=delta, pool=pool)
    f = 1.0 + kappa / 16.0 if kind == "offset" else 1.0
    what = "%s %s" % (name, shape)
    if kind != "tiny_var":
        return _judge(c, what, f)
    hip, t32 = _hip(c), _torch32(c)
    rest = torch.tensor([ch for ch in range(shape[1]) if ch != c.special])
    _judge(c, what + " [channel %d: sigma 1e-4 at 1]" % c.special, f, channels=torch.tensor([c.special]), hip=hip, t32=t32)
    _judge(c, what + " [the other channels]", f, channels=rest, hip=hip, t32=t32)


@pytest.mark.parametrize("shape,pool", B.SEQ_SHAPES, ids=["two_launch", "one_launch", "stem"])
def test_running_statistics_over_three_training_calls_and_an_evaluation(shape, pool):
    """groups = 3: nine momentum updates in group order with the unbiased n / (n - 1) variance, then an evaluation call that
    normalises with the result -- against the float64 chain after every call."""
    from shapeclipper_amd.functional import bn_act, bn_relu_maxpool
    cases = [B.make(shape, 3, pool=pool, seed=s) for s in range(4)]
    c0 = cases[0]
    bn_h, bn_t = _module(c0), _module(c0)
    g64, b64, rm, rv = c0.gamma.double(), c0.beta.double(), c0.rm0.double(), c0.rv0.double()
    fn = (lambda bn, x: bn_relu_maxpool(bn, x, groups=3)) if pool else (lambda bn, x: bn_act(bn, x, relu=True, groups=3))
    stock = lambda bn, x: torch.relu(torch.cat([bn(t) for t in x.chunk(3)], 0))
    bad = []

    def check(q, a, b, ref, what):
        eh, et = _rel(a, ref), _rel(b, ref)
        bar = max(B0[q], MARGIN * et)
        print("BN64 | sequence %s %s | %s | e_hip %.3e | e_torch %.3e | bar %.3e" % (shape, what, q, eh, et, bar))
        if not eh <= bar:
            bad.append("%s %s: e_hip %.3e > bar %.3e" % (what, q, eh, bar))
    with torch.no_grad():
        for k, c in enumerate(cases[:3]):
            x = c.x.cuda()
            fn(bn_h, x)
            stock(bn_t, x)
            _, _, _, _, rm, rv = B.forward64(c.x.double(), None, g64, b64, rm, rv, True, 3, True, pool)
            check("running_mean", bn_h.running_mean, bn_t.running_mean, rm, "call %d" % (k + 1))
            check("running_var", bn_h.running_var, bn_t.running_var, rv, "call %d" % (k + 1))
            assert int(bn_h.num_batches_tracked) == int(bn_t.num_batches_tracked) == 3 * (k + 1)
        bn_h.eval()
        bn_t.eval()
        x = cases[3].x.cuda()
        y_h, y_t = fn(bn_h, x), stock(bn_t, x)
        if pool:
            y_t = F.max_pool2d(y_t, 3, 2, 1)
        y64 = B.forward64(cases[3].x.double(), None, g64, b64, rm, rv, False, 3, True, pool)[0]
        check("y", y_h, y_t, y64, "evaluation")
        assert int(bn_h.num_batches_tracked) == 9 and _rel(bn_h.running_mean, rm) <= B0["running_mean"]       # untouched by the evaluation
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("shape,groups", [((1, 8, 1, 1), 1), ((3, 8, 1, 1), 3)])
@pytest.mark.parametrize("pool", [False, True])
def test_one_value_per_channel_and_group(shape, groups, pool):
    """Training: nn.BatchNorm2d's ValueError before any launch (the kernels would normalise with variance 0).  Evaluation: works."""
    from shapeclipper_amd.functional import bn_act, bn_relu_maxpool
    fn = (lambda bn, x: bn_relu_maxpool(bn, x, groups=groups)) if pool else (lambda bn, x: bn_act(bn, x, groups=groups))
    c = B.make(shape, groups, training=False, pool=pool)
    for bn in (_module(c).train(), nn.BatchNorm2d(8, track_running_stats=False).cuda().eval()):
        with _counting("sc_bn_act_forward", "sc_bn_relu_pool_forward") as calls:
            with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
                fn(bn, c.x.cuda())
        assert not calls
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            bn(c.x.cuda()[:1])                                       # the stock module's own refusal, same message
    _judge(c, "one value per group, evaluation %s pool%d" % (shape, pool))


@pytest.mark.parametrize("shape", [(4, 16, 8, 8), (8, 256, 14, 14)], ids=["two_launch", "one_launch"])
def test_non_finite_inputs_stay_in_their_channels(shape):
    """One NaN and one +Inf in different channels: exactly those channels are non-finite in y, dx, dgamma and the running
    statistics -- the same elements as in float64 -- and every other channel meets its bar."""
    base = B.make(shape, 1, relu=True, with_res=True, training=True)
    x = base.x.clone()
    x[1, 4, 2, 3] = float("nan")
    x[2, 7, 0, 1] = float("inf")
    c = B.Case(**dict(base.__dict__, x=x))
    ref, hip, t32 = B.reference(c), _hip(c), _torch32(c)
    clean = torch.tensor([ch for ch in range(shape[1]) if ch not in (4, 7)])
    for q in ("y", "dx", "dres", "dgamma", "dbeta", "running_mean", "running_var"):
        fin = torch.isfinite(ref[q])
        assert torch.equal(torch.isfinite(hip[q]).cpu(), fin), q
        dim = 1 if fin.dim() == 4 else 0
        assert bool(fin.index_select(dim, clean).all()), q
        if q not in ("dres", "dbeta"):            # sums of the masked dy itself: finite in every channel, in float64 too
            assert not bool(fin.index_select(dim, torch.tensor([4, 7])).any()), q
    _judge(c, "non-finite %s [clean channels]" % (shape,), channels=clean, hip=hip, t32=t32)


def test_strided_and_offset_views_give_the_contiguous_result():
    """A channel slice of a wider tensor (x and dy) and a view at a storage offset of one element go through ops._aligned: the same bits
    as the contiguous tensors.  Every view lies inside its storage."""
    from shapeclipper_amd.functional import bn_act
    c = B.make((4, 16, 8, 8), 2, relu=True, with_res=True, training=True)

    def run(x, res, dy):
        bn = _module(c)
        x, res = x.requires_grad_(True), res.requires_grad_(True)
        y = bn_act(bn, x, residual=res, relu=True, groups=2)
        y.backward(dy)
        return y.detach(), x.grad, res.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var

    def sliced(t):
        wide = torch.randn(4, 18, 8, 8, device="cuda")
        wide[:, 1:17] = t
        v = wide[:, 1:17]
        assert not v.is_contiguous()
        return v.detach()

    def shifted(t):
        buf = torch.zeros(t.numel() + 1, device="cuda")
        buf[1:] = t.reshape(-1)
        v = buf[1:].view(t.shape)
        assert v.is_contiguous() and v.storage_offset() % 4 == 1
        return v.detach()
    x, res, dy = c.x.cuda(), c.res.cuda(), c.cot.cuda()
    want = run(x.clone(), res.clone(), dy)
    for view in (sliced, shifted):
        got = run(view(x), view(res), view(dy))
        for a, b in zip(got, want):
            assert torch.equal(a, b), view.__name__


@pytest.mark.parametrize("pool", [False, True])
def test_zero_length_batch(pool):
    from shapeclipper_amd.functional import bn_act, bn_relu_maxpool
    bn = nn.BatchNorm2d(16).cuda().train()
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 1.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    x = torch.empty(0, 16, 8, 8, device="cuda")
    y = bn_relu_maxpool(bn, x) if pool else bn_act(bn, x)
    assert y.shape == ((0, 16, 4, 4) if pool else (0, 16, 8, 8))
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and int(bn.num_batches_tracked) == 0
