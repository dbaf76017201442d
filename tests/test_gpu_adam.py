"""The fused Adam / AdamW tail (csrc/adr_optim.hip adam_ema_kernel behind adr_opt_step_adam) and its wiring into
FusedTrainer(optimizer=...): the kernel against torch.optim.Adam / AdamW, the trainer's own step recomputed in
float64, the captured step against the eager one, and optimizer='auto'.

Accuracy criterion (tests 1 and 2). Truth is the float64 computation; the yardstick is the same computation in
float32 by torch. Per entry and step, max|kernel - truth| <= 4 * max|float32 torch - truth| + 2 ulp, the ulp taken
at the entry's largest truth magnitude of the array compared (parameter, first or second moment). The factor 4
covers the different but equally valid rounding order of the clip coefficient and the bias-correction scalars."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import ROOT
from gpu_util import load_recipe_into
from recipe import synthetic_images, synthetic_labels

pytestmark = pytest.mark.gpu
CFG = ROOT / "tests" / "configs" / "yolo11-701-YOLO-AD-Refine.yaml"

# round, tail and two-chunk edges of CHUNK = 4096 with 256 threads x U = 4, then one EMA-only entry
LENS = [1, 255, 1023, 1024, 1025, 4096, 4097, 300]
GROUPS = [0, 1, 2, 0, 1, 2, 0, 3]
LRS = [0.01, 0.003, 0.02]  # by group
WDS = [0.05, 0.0, 0.0]
BETA1, BETA2, EPS, MAX_NORM = 0.9, 0.999, 1e-8, 10.0
EMA_D = 0.875  # exact in fp32, and so is 1 - d, which the kernel forms in fp32 as the SGD kernel does
SENT = 12345.0  # guard element after every entry, on every array
CHUNK = 4096


def _ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _within(kern, f32, f64, what):
    """max|kern - f64| <= 4 * max|f32 - f64| + 2 ulp(max|f64|); all CPU tensors."""
    ek = float((kern.double() - f64).abs().max())
    et = float((f32.double() - f64).abs().max())
    bound = 4 * et + 2 * _ulp(f64.abs().max())
    print(f"{what}: kernel err {ek:.3e}, float32 torch err {et:.3e}, bound {bound:.3e}")
    assert ek <= bound, (what, ek, et, bound)


def _hyper_vals(t, decoupled):
    bc1 = 1 - BETA1 ** t
    bc2 = 1 - BETA2 ** t
    return LRS + WDS + [1 - BETA1, BETA2, 1 - BETA2, EPS] + [lr / bc1 for lr in LRS] + [bc2 ** 0.5, EMA_D,
                                                                                         1.0 if decoupled else 0.0]


def _kernel_vs_torch(name, grad_scale, zeros, use_ema):
    from adrefine import kernels as K
    from adrefine.engine.trainer import _CHUNK, _ENTRY
    from adrefine.native import lib
    offs = np.concatenate([[0], np.cumsum([n + 1 for n in LENS])])  # each entry is followed by its guard
    T = int(offs[-1])
    inside = torch.zeros(T, dtype=torch.bool)
    for off, n in zip(offs, LENS):
        inside[off:off + n] = True
    gen = torch.Generator().manual_seed(7)

    def arena(vals):
        return torch.where(inside, vals, torch.full((T,), SENT))

    p0 = arena(torch.randn(T, generator=gen))
    e0 = arena(torch.randn(T, generator=gen))
    P, E, G = p0.cuda(), e0.cuda(), arena(torch.zeros(T)).cuda()
    ST = torch.cat([arena(torch.zeros(T))] * 2).cuda()  # first moments, then second moments at + T
    tab = np.zeros(len(LENS), dtype=_ENTRY)
    chunks = []
    for ei, (off, n, grp) in enumerate(zip(offs, LENS, GROUPS)):
        tab["p"][ei] = P.data_ptr() + 4 * off
        tab["g"][ei] = G.data_ptr() + 4 * off if grp < 3 else 0
        tab["b"][ei] = ST.data_ptr() + 4 * off
        tab["e"][ei] = E.data_ptr() + 4 * off if use_ema else 0
        tab["n"][ei] = n
        tab["grp"][ei] = grp
        chunks += [(ei, 0, s, min(CHUNK, n - s)) for s in range(0, n, CHUNK)]
    assert len(chunks) == len(LENS) + 1  # the 4097 entry spans two chunks
    tab_dev = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    chunks_dev = torch.from_numpy(np.array(chunks, dtype=_CHUNK).view(np.uint8).copy()).cuda()
    partial = torch.empty(len(chunks), dtype=torch.float32, device="cuda")
    norm = torch.zeros(1, dtype=torch.float32, device="cuda")
    hyper = torch.zeros(16, dtype=torch.float32, device="cuda")

    upd = [ei for ei, grp in enumerate(GROUPS) if grp < 3]
    sl = [slice(int(offs[ei]), int(offs[ei]) + LENS[ei]) for ei in range(len(LENS))]
    cls = getattr(torch.optim, name)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(p0[sl[ei]].to(dt).clone()) for ei in upd]
        opt = cls([{"params": [p], "lr": LRS[GROUPS[ei]], "weight_decay": WDS[GROUPS[ei]]} for p, ei in zip(ps, upd)],
                  betas=(BETA1, BETA2), eps=EPS, foreach=False)
        ref[dt] = (ps, opt)

    ema_prev = e0.clone()
    for t in (1, 2, 3):
        g = grad_scale * torch.randn(T, generator=gen)
        if zeros:
            g[::7] = 0.0
        g[sl[-1]] = 0.0  # the EMA-only entry has no gradient: nothing there for the kernel to zero
        G.copy_(arena(g))
        vals = _hyper_vals(t, name == "AdamW")
        arr = (ctypes.c_float * 16)(*vals)
        lib.adr_set_f32(K.fptr(hyper), ctypes.cast(arr, ctypes.c_void_p), 16, K.stream())
        lib.adr_opt_step_adam(K.fptr(tab_dev), K.fptr(chunks_dev), len(chunks), K.fptr(partial), MAX_NORM,
                              K.fptr(hyper), T, K.fptr(norm), K.stream())
        torch.cuda.synchronize()
        tn = {}
        for dt, (ps, opt) in ref.items():
            for p, ei in zip(ps, upd):
                p.grad = g[sl[ei]].to(dt).clone()
            tn[dt] = torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
            opt.step()
        tn64 = float(tn[torch.float64])
        assert (tn64 > MAX_NORM) == (grad_scale >= 1.0)  # the case this run is meant to be
        assert abs(float(norm) - tn64) <= 1e-6 * tn64, (float(norm), tn64)
        Pc, Gc, STc, Ec = P.cpu(), G.cpu(), ST.cpu(), E.cpu()
        for arr_c, what in ((Pc, "p"), (Gc, "g"), (STc[:T], "m"), (STc[T:], "v"), (Ec, "ema")):
            assert bool((arr_c[~inside] == SENT).all()), f"guard element of {what} overwritten"
        assert not Gc[inside].any()  # zero_grad
        for k, ei in enumerate(upd):
            (p64, o64), (p32, o32) = ref[torch.float64], ref[torch.float32]
            tag = f"{name} step {t} entry n={LENS[ei]} g{GROUPS[ei]}"
            _within(Pc[sl[ei]], p32[k].detach(), p64[k].detach(), tag + " param")
            _within(STc[:T][sl[ei]], o32.state[p32[k]]["exp_avg"], o64.state[p64[k]]["exp_avg"], tag + " exp_avg")
            _within(STc[T:][sl[ei]], o32.state[p32[k]]["exp_avg_sq"], o64.state[p64[k]]["exp_avg_sq"],
                    tag + " exp_avg_sq")
        # the EMA-only entry: parameter bitwise untouched, no moments
        assert torch.equal(Pc[sl[-1]], p0[sl[-1]])
        assert not STc[:T][sl[-1]].any() and not STc[T:][sl[-1]].any()
        if use_ema:  # every entry, the EMA-only one included: d * ema + (1 - d) * p of the updated parameter
            want = EMA_D * ema_prev.double() + (1 - EMA_D) * Pc.double()
            tol = 4 * 2.0 ** -24 * (EMA_D * ema_prev.abs() + (1 - EMA_D) * Pc.abs()).double()  # three fp32 roundings
            assert bool(((Ec.double() - want).abs() <= tol)[inside].all())
            assert not torch.equal(Ec[sl[-1]], ema_prev[sl[-1]])
            ema_prev = Ec.clone()
        else:
            assert torch.equal(Ec, e0)


@pytest.mark.parametrize("name", ["AdamW", "Adam"])
@pytest.mark.parametrize("grad_scale,zeros", [(1.0, False), (0.01, True)], ids=["clipped", "unclipped_zeros"])
def test_kernel_matches_torch(name, grad_scale, zeros):
    """Three steps over entries of 1 ... 4097 elements in groups 0-2 with three lrs and weight decay on group 0, one
    EMA-only entry; total norm above max_norm (clipped) and below it with exact-zero gradient elements."""
    _kernel_vs_torch(name, grad_scale, zeros, use_ema=True)


def test_kernel_without_ema():
    _kernel_vs_torch("AdamW", 1.0, False, use_ema=False)


def test_entry_checks_arguments():
    from adrefine import kernels as K
    from adrefine.native import lib
    t = torch.zeros(64, device="cuda")
    for args in ((K.fptr(t), K.fptr(t), 0, K.fptr(t), 10.0, K.fptr(t)),
                 (None, K.fptr(t), 1, K.fptr(t), 10.0, K.fptr(t)),
                 (K.fptr(t), None, 1, K.fptr(t), 10.0, K.fptr(t)),
                 (K.fptr(t), K.fptr(t), 1, K.fptr(t), 10.0, None)):
        with pytest.raises(RuntimeError, match="opt_step_adam"):
            lib.adr_opt_step_adam(*args, 0, None, K.stream())


# ---- trainer -------------------------------------------------------------------------------------------------

def _trainer(**kw):
    from adrefine.engine.trainer import FusedTrainer
    from adrefine.nn.tasks import DetectionModel
    m = DetectionModel(str(CFG))
    load_recipe_into(m)
    return FusedTrainer(m.cuda(), nbs=2, batch_size=2, **kw)


def _batch(seed):
    return {"img": synthetic_images(2, 320, seed=seed).cuda(), **synthetic_labels(2, 80, seed=seed + 1)}


def test_trainer_step_is_adamw_of_its_own_moments():
    """Two eager AdamW steps in the warm-up (nb = 10: the bias group's lr differs from the weights'). The second
    step is recomputed in float64 from the trainer's post-step moments and the schedule's scalars:
    p_after = p_before * (1 - lr * wd) - step_size * m / (sqrt(v) / bc2_sqrt + eps), wd on g0 only."""
    from adrefine.engine.trainer import param_groups
    tr = _trainer(optimizer="AdamW", lr0=0.002, momentum=0.9, nb=10, warmup_bias_lr=0.01)
    init = {k: v.detach().clone() for k, v in tr.model.named_parameters()}
    tr.step(_batch(0))
    torch.cuda.synchronize()
    before = {k: v.detach().cpu().clone() for k, v in tr.model.named_parameters()}
    ema_prev = {k: v.cpu().clone() for k, v in tr.ema_state_dict().items()}
    tr.step(_batch(5))
    torch.cuda.synchronize()
    assert tr.opt_steps == 2 and tr.updates == 2 and not tr.grad.any()
    lrs, beta1, _ = tr.sched.at(1)
    assert beta1 == 0.9 and lrs[2] != lrs[0] and lrs[0] > 0 and tr.lr == lrs
    ss, bc2_sqrt = [lr / (1 - 0.9 ** 2) for lr in lrs], (1 - 0.999 ** 2) ** 0.5  # torch's scalars for step 2
    ent = {name: (ei, t, grp) for ei, (name, t, grp, isp) in enumerate(tr.entries) if isp}
    used = [[n for n, p in g if getattr(p, "_adr_used", False)] for g in param_groups(tr.model)]
    assert all(used)
    for grp in (0, 1, 2):
        name = used[grp][0]
        ei, t, g = ent[name]
        assert g == grp
        sl = slice(tr._goff[ei], tr._goff[ei] + t.numel())
        m, v = tr.mom[sl].cpu(), tr.sq[sl].cpu()
        assert m.any() and v.any()
        pb = before[name].reshape(-1)
        wd = tr.wd if grp == 0 else 0.0

        def formula(dt):
            f = lambda x: torch.tensor(x, dtype=dt)  # noqa: E731 - a Python float rounded once, as a torch scalar
            denom = (v.to(dt).sqrt() / f(bc2_sqrt)) + f(tr.eps)
            return pb.to(dt) * f(1 - lrs[grp] * wd) - f(ss[grp]) * (m.to(dt) / denom)

        _within(t.detach().cpu().reshape(-1), formula(torch.float32), formula(torch.float64), f"g{grp} {name}")
        assert not torch.equal(t.detach().cpu().reshape(-1), pb)
    # a parameter that never receives a gradient: bitwise unchanged, moments zero
    idle = [(n, ei, t) for n, (ei, t, _) in ent.items() if not getattr(t, "_adr_used", False)]
    assert idle
    for n, ei, t in idle:
        sl = slice(tr._goff[ei], tr._goff[ei] + t.numel())
        assert torch.equal(t.detach(), init[n]) and not tr.mom[sl].any() and not tr.sq[sl].any()
    # EMA of one tensor with the trainer's d for its second update
    d = tr.ema_decay * (1 - math.exp(-2 / tr.ema_tau))
    k = used[0][0]
    want = d * ema_prev[k].double() + (1 - d) * ent[k][1].detach().cpu().double()
    got = tr.ema_state_dict()[k].cpu().double()
    tol = 4 * 2.0 ** -24 * (d * ema_prev[k].abs() + (1 - d) * ent[k][1].detach().cpu().abs()).double()
    assert bool(((got - want).abs() <= tol + 1e-7 * want.abs()).all())  # d itself is rounded to fp32: 6e-8 relative


def _pdiff(a, b):
    sa, sb = a.model.state_dict(), b.model.state_dict()
    return max(float((sa[k] - sb[k]).abs().max()) for k in sa if sa[k].dtype.is_floating_point)


def test_graph_step_matches_eager_adamw():
    """tests/test_gpu_graph.py's criterion for the SGD step (10 x the eager-eager spread + 2e-4), applied to the
    parameters, both moment arenas and the EMA of an AdamW trainer captured after its first eager step. A capture
    that froze step 2's bias corrections would scale steps 3 and 4 by 0.19 / 0.271 and 0.19 / 0.344."""
    seq = [_batch(0), _batch(0), _batch(5), _batch(0)]

    def run(graph):
        tr = _trainer(optimizer="AdamW", lr0=0.002, momentum=0.9)
        out = [tr.step(seq[0]).clone()]
        if graph:
            tr.capture(seq[1], max_targets=100)
        out += [tr.step(b).clone() for b in seq[1:]]
        torch.cuda.synchronize()
        return tr, out

    e1, o1 = run(False)
    e2, o2 = run(False)
    g, og = run(True)
    assert g.opt_steps == e1.opt_steps == 4
    for a, b, c in zip(o1, og, o2):
        assert float((a - b).abs().max()) <= 10 * float((a - c).abs().max()) + 2e-4 * float(a.abs().max()), (a, b, c)
    spread = _pdiff(e1, e2)
    d = _pdiff(e1, g)
    print(f"eager-eager max |dparam| {spread:.3e}, eager-graph {d:.3e}")
    assert d <= 10 * spread + 2e-4, (d, spread)
    for what in ("mom", "sq"):
        sp = float((getattr(e1, what) - getattr(e2, what)).abs().max())
        dd = float((getattr(e1, what) - getattr(g, what)).abs().max())
        print(f"{what}: eager-eager {sp:.3e}, eager-graph {dd:.3e}")
        assert dd <= 10 * sp + 2e-4, (what, dd, sp)
    ee, eg = e1.ema_state_dict(), g.ema_state_dict()
    assert max(float((ee[k] - eg[k]).abs().max()) for k in ee) <= 10 * spread + 2e-4
    # the replayed tail read step 4's scalars from device memory
    ss, bc2_sqrt = [0.002 / (1 - 0.9 ** 4)] * 3, (1 - 0.999 ** 4) ** 0.5
    assert torch.equal(g.hyper[10:14].cpu(), torch.tensor(ss + [bc2_sqrt], dtype=torch.float32))


def test_auto_builds_adamw_and_steps():
    from adrefine.engine.trainer import resolve_optimizer
    tr = _trainer(optimizer="auto", iterations=500, nb=10)
    nc = tr.model.model[-1].nc
    name, lr0, mom, wb = resolve_optimizer("auto", 0.01, 0.937, 0.1, nc, 500)
    assert (tr.optimizer, tr.sched.lr0, tr.momentum, tr.sched.warmup_bias_lr) == (name, lr0, mom, wb)
    assert name == "AdamW" and tr.adam and wb == 0.0
    p0 = tr.model.state_dict()["model.0.conv.weight"].clone()
    tr.step(_batch(0))
    torch.cuda.synchronize()
    assert tr.opt_steps == 1 and tr.sq.any() and tr.mom.any()
    # first-step scalars: every lr warms up from 0 (warmup_bias_lr 0), beta1 0.9 from batch 0
    want = [0.0] * 3 + [tr.wd, 0.0, 0.0, 1 - mom, 0.999, 1 - 0.999, 1e-8, 0.0, 0.0, 0.0, (1 - 0.999) ** 0.5,
            tr.ema_decay * (1 - math.exp(-1 / tr.ema_tau)), 1.0]
    assert torch.equal(tr.hyper.cpu(), torch.tensor(want, dtype=torch.float32))
    assert torch.equal(tr.model.state_dict()["model.0.conv.weight"], p0)  # lr 0 at ni = 0
    tr.step(_batch(5))
    torch.cuda.synchronize()
    assert tr.opt_steps == 2 and tr.lr[0] == pytest.approx(lr0 * tr.sched.lf(0) / 100, rel=1e-12)
    assert not torch.equal(tr.model.state_dict()["model.0.conv.weight"], p0)
