"""The fused loss takes the reference's raw inputs: full-size masks, pooled inside the kernels, and per-view weights.

add_proj_loss (dpc/models/model_pc_to.py:339-385) average-pools inputs["masks"] to the silhouette size with
nn.AvgPool2d(gt_size // pred_size), and with cfg.variable_num_views proj_loss_pose_candidates / add_student_loss weight every
sample by inputs["valid_samples"] (:432-436, 461-464, 480).  The contract (include/dpc_render.h, dpc_project_loss_fwd):

    gt[s,y,x] = (sum_{i<f} sum_{j<f} masks[s, f*y+i, f*x+j]) / (f*f)     -- the bits of F.avg_pool2d(masks, f)
    sse[c]    = sum_pix (gt[c/K] - proj[c])^2                            -- unweighted
    winner[s] = first argmin_k sse[s*K+k]                                -- unweighted
    loss      = sum_s w_s^2 sse[s*K + winner[s]] / S
    student   = sum_s w_s (1 - <t,s>^2 / (|t|^2 |s|^2)) / S * weight     -- w not squared

CPU part: the restatement below against the reference's own add_proj_loss / add_student_loss (fixture F14,
tests/golden/make_golden_pooled.py), the harness's weighted student loss, the ABI number and the refusals that come before
any launch.  GPU part: full-size masks give the same bits as F.avg_pool2d + the pre-pooled call on every path, and the
weighted loss matches the oracle's fp64 chain + the restatement under the parity rule of tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ the restatement
def pooled(masks, f):
    """[S,1,f*H,f*W] -> [S,H,W,1] (nn.AvgPool2d(f) + the permute of add_proj_loss)."""
    return (F.avg_pool2d(masks, f) if f > 1 else masks).permute(0, 2, 3, 1)


def weighted_loss(gt, pred, K, w=None):
    """gt [S,H,W,1], pred [S*K,H,W,1] -> (sum_s w_s^2 min_k sse / S, winners): proj_loss_pose_candidates with
    variable_num_views (K = 1 is the min-of-1 case)."""
    S = gt.shape[0]
    sse = ((gt.repeat_interleave(K, 0) - pred) ** 2).sum((1, 2, 3)).reshape(S, K)
    win = sse.argmin(1)
    best = sse.gather(1, win[:, None])[:, 0]
    if w is not None:
        best = best * w.to(best.dtype) ** 2
    return best.sum() / S, win


@pytest.fixture(scope="module")
def f14(golden):
    return golden("f14_pooled_loss.npz")


@pytest.mark.parametrize("f", [2, 3])
def test_restatement_matches_the_reference(f14, f):
    """The restatement the GPU tests compare against IS the reference's add_proj_loss (F14: K = 4, weights 0 / 0.5 / 1)."""
    sfx = "_f%d" % f
    K = int(f14["K"])
    masks, w = torch.from_numpy(f14["masks" + sfx]), torch.from_numpy(f14["weights"])
    pred = torch.from_numpy(f14["pred" + sfx]).requires_grad_(True)
    loss, win = weighted_loss(pooled(masks, f), pred, K, w)
    loss.backward()
    assert np.array_equal(win.numpy(), f14["min_loss" + sfx])
    assert abs(float(loss.detach()) - float(f14["loss" + sfx])) <= 1e-12 * max(1.0, abs(float(f14["loss" + sfx])))
    assert np.abs(pred.grad.numpy() - f14["dpred" + sfx]).max() <= 1e-12


@pytest.mark.parametrize("f", [2, 3])
def test_student_loss_weights(f14, f):
    """dpc.harness.student_loss(..., weights=valid_samples) = the reference's add_student_loss with variable_num_views."""
    from dpc.harness import student_loss

    sfx = "_f%d" % f
    K = int(f14["K"])
    student = torch.from_numpy(f14["student" + sfx]).requires_grad_(True)
    loss = student_loss(torch.from_numpy(f14["poses" + sfx]), student, torch.from_numpy(f14["min_loss" + sfx]), K, 1.0,
                        weights=torch.from_numpy(f14["weights"]))
    loss.backward()
    ref = float(f14["student_loss" + sfx])
    assert abs(float(loss.detach()) - ref) <= 1e-12 * max(1.0, abs(ref))
    assert np.abs(student.grad.numpy() - f14["dstudent" + sfx]).max() <= 1e-12


def test_abi_version_is_15():
    from dpc.render import _native

    assert _native.lib().dpc_abi_version() == 15 == _native.ABI_VERSION


def _cpu_call(G=16, S=2, K=1):
    import dpc.render as R

    cfg = dict(vox_size=G, pc_gauss_kernel_size=11)
    pc, q = torch.zeros(S * K, 10, 3), torch.ones(S * K, 4)
    kern = R.smoothing_kernel(type("C", (dict,), {"__getattr__": dict.__getitem__})(cfg), 1.0)
    cfg = type("C", (dict,), {"__getattr__": dict.__getitem__})(cfg)
    return lambda gt, w=None: R.pointcloud_project_loss(cfg, pc, q, None, None, kern, gt=gt, num_candidates=K,
                                                         valid_samples=w)


@pytest.mark.parametrize("shape,what", [((2, 1, 40, 40), "not an integer multiple"), ((2, 1, 8, 8), "smaller"),
                                        ((2, 40, 40, 1), "not an integer multiple"), ((2, 1, 32, 48), "not an integer")])
def test_masks_of_the_wrong_size_are_refused(shape, what):
    """Mask sides below the silhouette's (the reference asserts) or not a multiple of it: ValueError before any launch."""
    import dpc.render as R

    call = _cpu_call()
    with pytest.raises(ValueError, match=what):
        call(torch.zeros(shape))
    with pytest.raises(ValueError, match=what):
        R.silhouette_loss(torch.zeros(2, 16, 16, 1), torch.zeros(shape))


@pytest.mark.parametrize("wshape", [(2, 1), (3,), (1, 2)])
def test_weights_of_the_wrong_shape_are_refused(wshape):
    import dpc.render as R

    call = _cpu_call()
    with pytest.raises(ValueError, match="valid_samples"):
        call(torch.zeros(2, 1, 32, 32), torch.ones(wshape))
    with pytest.raises(ValueError, match="valid_samples"):
        R.silhouette_loss(torch.zeros(2, 16, 16, 1), torch.zeros(2, 1, 32, 32), 1, torch.ones(wshape))


def test_bad_gt_factor_is_a_shape_error_before_any_launch():
    """gt_factor < 1, or masks sides beyond 1024: DPC_ERR_SHAPE from every entry point, returned before anything is launched
    or dereferenced (no device needed)."""
    from dpc.render import _native as N

    L = N.lib()
    P = N.DpcParams(B=2, N=10, D=32, H=32, W=32, taps_xy=0, taps_z=0, camera_distance=2.0, focal_length=1.875,
                    clip_val=1e-5, max_depth=10.0, point_replicas=1)
    host = (ctypes.c_float * 4)()
    loss = ctypes.cast(host, ctypes.c_void_p)   # a non-NULL loss pointer: the checks must not get as far as using it
    for gf in (0, -1, 33):
        fwd = L.dpc_project_loss_fwd(ctypes.byref(P), *([None] * 8), gf, None, 1, *([None] * 8), loss, None, None, None, None,
                                     None)
        bwd = L.dpc_project_loss_bwd(ctypes.byref(P), *([None] * 13), gf, None, 1, None, None, 0, None, None, None, None)
        step = L.dpc_project_loss_step(ctypes.byref(P), *([None] * 8), gf, None, 1, *([None] * 15))
        assert fwd == bwd == step == N.DPC_ERR_SHAPE, (gf, fwd, bwd, step)
    for gf, H in ((0, 16), (-2, 16), (65, 16)):
        assert L.dpc_silhouette_loss(None, gf, None, None, 2, 1, H, H, None, None, None, None) == N.DPC_ERR_SHAPE


# ------------------------------------------------------------------------------------------------ GPU
def _masks(S, side, seed, binary):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(S, 1, side, side, generator=g)
    return (m > 0.5).float() if binary else m


def _weights(S):
    return torch.tensor([0.0, 1.0, 0.5, 2.0] * ((S + 3) // 4))[:S]


def _fused(R, cfg, kern, pc, q, s, gt, K, w=None, point_index=None):
    """One pointcloud_project_loss + backward on fresh leaves: (loss, proj, winner, dpc, dq, ds)."""
    gp, gq, gs = (x.detach().clone().cuda().requires_grad_(True) for x in (pc, q, s))
    loss, out, win = R.pointcloud_project_loss(cfg, gp, gq, None, None, kern, scaling_factor=gs, gt=gt, num_candidates=K,
                                               point_index=point_index, valid_samples=w)
    (1.5 * loss).backward()
    torch.cuda.synchronize()
    return loss.detach(), out["proj"].detach(), win, gp.grad, gq.grad, gs.grad


NAMES = ("loss", "proj", "winner", "dpc", "dq", "ds")


def _assert_equal(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), "%s: %s differs (max %.3e)" % (what, name, (x.double() - y.double()).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("K,R_,indexed", [(1, 1, False), (4, 1, False), (1, 2, False), (4, 4, True)])
@pytest.mark.parametrize("binary", [True, False])
def test_full_size_masks_give_the_pooled_bits(f, K, R_, indexed, binary):
    """Masks [S,1,f*G,f*G] pooled inside the kernels == F.avg_pool2d + the pre-pooled call, bit for bit: loss, silhouettes,
    winners and every gradient; K = 1 (pooling in k_zcol_fwdbwd) and K = 4 (k_zcol_fwd + the backward's ray_grad), shared
    point sets and per-cloud point subsets."""
    import dpc.render as R
    from oracle import dpc_oracle as O

    S, N, G = 4, 700, 32
    B = S * K
    cfg = O.Cfg(vox_size=G, pc_gauss_kernel_size=11)
    kern = R.smoothing_kernel(cfg, 1.1)
    pc, q, s, _, _, _ = O.synth_inputs(B, N, G, 140 + f + K)
    idx = None
    assert B % R_ == 0
    if R_ > 1:
        pc = pc[::R_]   # B / R_ point sets: the renderer runs with point_replicas = R_
    if indexed:
        g = torch.Generator().manual_seed(5)
        idx = torch.stack([torch.randperm(N, generator=g)[:N // 2] for _ in range(B)]).int().cuda()
    masks = _masks(S, f * G, 7 * f, binary).cuda()
    a = _fused(R, cfg, kern, pc, q, s, masks, K, point_index=idx)
    b = _fused(R, cfg, kern, pc, q, s, F.avg_pool2d(masks, f).permute(0, 2, 3, 1).contiguous(), K, point_index=idx)
    _assert_equal(a, b, "f=%d K=%d R=%d" % (f, K, R_))
    # NCHW and NHWC layouts of the same masks are the same bytes (one channel)
    c = _fused(R, cfg, kern, pc, q, s, masks.permute(0, 2, 3, 1), K, point_index=idx)
    _assert_equal(a, c, "NHWC masks")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 8])
def test_step_plan_pools_masks_bit_for_bit_at_c2(K):
    """ProjectLossStep at c2 size (B = 32, N = 8000, 64^3, sigma_rel 0.64): run(pc, q, s, masks 128^2) == run on the
    F.avg_pool2d'ed masks, bit for bit, with and without weights (all ones = no weights, too)."""
    import dpc.render as R
    from oracle import dpc_oracle as O

    B, N, G = 32, 8000, 64
    S = B // K
    cfg = O.Cfg(vox_size=G, pc_gauss_kernel_size=21)
    plan = R.project_loss_step(cfg, R.smoothing_kernel(cfg, 0.64), B, N, "cuda", num_candidates=K)
    pc, q, s, _, _, _ = O.synth_inputs(B, N, G, 2)
    pc, q, s = pc.cuda(), q.cuda(), s.cuda()
    masks = _masks(S, 2 * G, 11, True).cuda()
    pre = F.avg_pool2d(masks, 2).permute(0, 2, 3, 1).contiguous()

    def run(gt, w=None):
        loss = plan.run(pc, q, s, gt, valid_samples=w)
        torch.cuda.synchronize()
        return tuple(x.clone() for x in (loss, plan.proj, plan.winner, plan.dpc, plan.dq, plan.ds))

    a, b = run(masks), run(pre)
    assert plan.gt_factor == 1
    _assert_equal(a, b, "step plan, K=%d" % K)
    w = _weights(S).cuda()
    _assert_equal(run(masks, w), run(pre, w), "step plan, weighted")
    _assert_equal(run(masks, torch.ones(S, device="cuda")), a, "step plan, weights all ones")
    ref, _ = weighted_loss(pre.double(), b[1].double(), K, w.double())
    out = run(masks, w)
    assert abs(float(out[0]) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    plan.run(pc, q, s, masks)   # binding the masks fixes f
    assert plan.gt_factor == 2


@pytest.mark.gpu
def test_staged_fallback_and_silhouette_loss_pool_and_weight():
    """Taps longer than the fused kernels take: pointcloud_project_fast + silhouette_loss, which get the raw masks and the
    weights (k_silhouette_loss pools and weights them) -- bit for bit the pre-pooled call; and silhouette_loss itself."""
    import dpc.render as R
    from oracle import dpc_oracle as O

    S, K, G = 3, 2, 32
    cfg = O.Cfg(vox_size=G, pc_gauss_kernel_size=41)
    kern = R.smoothing_kernel(cfg, 8.0)
    pc, q, s, _, _, _ = O.synth_inputs(S * K, 400, G, 99)
    w = _weights(S).cuda()
    for f in (2, 3):
        masks = _masks(S, f * G, f, False).cuda()
        pre = F.avg_pool2d(masks, f).permute(0, 2, 3, 1).contiguous()
        a = _fused(R, cfg, kern, pc, q, s, masks, K, w)
        b = _fused(R, cfg, kern, pc, q, s, pre, K, w)
        _assert_equal(a, b, "staged fallback f=%d" % f)
        ref, rwin = weighted_loss(pre.double(), a[1].double(), K, w.double())
        assert torch.equal(a[2].long().cpu(), rwin.cpu())
        assert abs(float(a[0]) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    for f in (2, 3, 4):
        masks = _masks(4, f * 16, 20 + f, f == 2).cuda()
        pre = F.avg_pool2d(masks, f).permute(0, 2, 3, 1).contiguous()
        pred = torch.rand(8, 16, 16, 1, generator=torch.Generator().manual_seed(f)).cuda()
        for w in (None, _weights(4).cuda()):
            pa, pb = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
            la, wa = R.silhouette_loss(pa, masks, 2, w)
            lb, wb = R.silhouette_loss(pb, pre, 2, w)
            la.backward()
            lb.backward()
            assert torch.equal(la, lb) and torch.equal(wa, wb) and torch.equal(pa.grad, pb.grad)
            ref, rwin = weighted_loss(pre.double(), pred.double(), 2, None if w is None else w.double())
            assert torch.equal(wa.long().cpu(), rwin.cpu())
            assert abs(float(la) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))


@pytest.mark.gpu
@pytest.mark.parametrize("K,f,G", [(1, 1, 32), (1, 2, 64), (1, 3, 32), (4, 2, 32), (4, 3, 64), (4, 1, 64), (8, 1, 32),
                                   (8, 2, 32), (8, 3, 32)])
def test_weighted_loss_vs_oracle(K, f, G):
    """Weights {0, 1, 0.5, 2}: device loss, silhouettes, winners and gradients vs the oracle's fp64 chain + the restatement,
    under 1e-5 * max(1, max|ref|); a zero-weight sample's clouds get exactly zero gradients."""
    import dpc.render as R
    from oracle import dpc_oracle as O
    from test_gpu_parity import TOL, close

    O.EXACT_POSE_GRADIENT = True
    try:
        S, N = 4, 600
        B = S * K
        cfg = O.Cfg(vox_size=G, pc_gauss_kernel_size=11)
        pc, q, s, _, _, _ = O.synth_inputs(B, N, G, 300 + 10 * K + f)
        masks = _masks(S, f * G, 40 + f, K != 4)
        w = _weights(S)
        leaf = lambda x: x.clone().requires_grad_(True)
        cp, cq, cs = leaf(pc), leaf(q), leaf(s)
        ref = O.pointcloud_project_fast(cfg, cp, cq, None, None, O.smoothing_kernel(cfg, 1.1), scaling_factor=cs)
        rloss, rwin = weighted_loss(pooled(masks.double(), f), ref["proj"], K, w.double())
        (1.5 * rloss).backward()
        loss, proj, win, dpc, dq, ds = _fused(R, cfg, R.smoothing_kernel(cfg, 1.1), pc, q, s, masks.cuda(), K, w.cuda())
        what = "K=%d f=%d G=%d" % (K, f, G)
        assert np.array_equal(win.cpu().numpy(), rwin.numpy()), what
        close(loss, rloss, TOL, "weighted loss " + what)
        close(proj, ref["proj"], TOL, "weighted proj " + what)
        close(dpc, cp.grad, TOL, "weighted dpc " + what)
        close(dq, cq.grad, TOL, "weighted dq " + what)
        close(ds, cs.grad, TOL, "weighted ds " + what)
        zero = (w == 0).repeat_interleave(K).cuda()
        assert dpc[zero].abs().max().item() == 0.0 and dq[zero].abs().max().item() == 0.0 and ds[zero].abs().max().item() == 0.0
        assert dpc[~zero].abs().max().item() > 0.0
    finally:
        O.EXACT_POSE_GRADIENT = False


@pytest.mark.gpu
def test_weighted_pooled_loss_at_c5():
    """c5 at full size: 16 samples x K = 8 candidates of one shared point set each, 8000 points, 64^3, masks 128^2 pooled in
    the kernels, weights with zeros: loss and winners vs the restatement on the device's silhouettes, the pooled bits vs
    F.avg_pool2d, zero gradients for zero-weight samples and losers, and one weighted sample's gradients vs the oracle."""
    import dpc.render as R
    from oracle import dpc_oracle as O
    from test_gpu_parity import TOL, close

    S, K, N, G = 16, 8, 8000, 64
    B = S * K
    cfg = O.Cfg(vox_size=G, pc_gauss_kernel_size=21)
    kern = R.smoothing_kernel(cfg, 0.64)
    base, _, sb, _, _, _ = O.synth_inputs(S, N, G, 505)
    s = sb.repeat_interleave(K, dim=0)
    q = O.synth_inputs(B, 1, G, 506)[1]
    masks = _masks(S, 2 * G, 507, True).cuda()
    w = _weights(S).cuda()
    a = _fused(R, cfg, kern, base, q, s, masks, K, w)
    b = _fused(R, cfg, kern, base, q, s, F.avg_pool2d(masks, 2).permute(0, 2, 3, 1).contiguous(), K, w)
    _assert_equal(a, b, "c5")
    loss, proj, win, dpc, dq, ds = a
    rloss, rwin = weighted_loss(pooled(masks.double().cpu(), 2), proj.double().cpu(), K, w.double().cpu())
    assert np.array_equal(win.cpu().numpy(), rwin.numpy())
    close(loss, rloss, TOL, "c5 weighted loss")
    zero_sets = (w == 0)
    assert dpc[zero_sets].abs().max().item() == 0.0
    assert dq[(w == 0).repeat_interleave(K)].abs().max().item() == 0.0
    smp = 3   # weight 2
    O.EXACT_POSE_GRADIENT = True
    try:
        sl = slice(smp * K, (smp + 1) * K)
        cp = base[smp:smp + 1].repeat_interleave(K, dim=0).clone().requires_grad_(True)
        cq, cs = q[sl].clone().requires_grad_(True), s[sl].clone().requires_grad_(True)
        ref = O.pointcloud_project_fast(cfg, cp, cq, None, None, O.smoothing_kernel(cfg, 0.64), scaling_factor=cs)
        l1, w1 = weighted_loss(pooled(masks[smp:smp + 1].double().cpu(), 2), ref["proj"], K, w[smp:smp + 1].double().cpu())
        (1.5 * l1 / S).backward()
        assert w1.item() == rwin[smp].item()
        close(proj[sl], ref["proj"], TOL, "c5 proj vs oracle")
        close(dpc[smp], cp.grad.sum(0), TOL, "c5 weighted dpc vs oracle")
        close(dq[sl], cq.grad, TOL, "c5 weighted dq vs oracle")
    finally:
        O.EXACT_POSE_GRADIENT = False


# ------------------------------------------------------------------------------------------------ harness
@pytest.mark.gpu
def test_harness_weighted_loss():
    """TrainStep.loss with valid_samples containing a 0 = the weighted restatement of its own pieces (projections, pooled
    masks, winners, student term); valid_samples None and all ones: the same loss and parameter gradients, bit for bit."""
    import json
    import os

    from dpc.harness import TrainStep, student_loss
    from test_gpu_parity import TOL, close

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    cfg = type("C", (dict,), {"__getattr__": dict.__getitem__})(json.load(open(os.path.join(golden, "f10_config.json"))))
    g = np.load(os.path.join(golden, "f10_full_step.npz"))
    state = {k[len("state/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}
    dev = torch.device("cuda")
    images, masks = torch.from_numpy(g["images"]).to(dev), torch.from_numpy(g["masks"]).to(dev)
    M, K = masks.shape[0], cfg.pose_predict_num_candidates
    step = TrainStep(cfg, dev)
    step.load_reference_state(state)

    heads = ("points_1", "poses", "pose_student", "scaling_factor")   # what the renderer and the student loss differentiate

    def run(w):
        np.random.seed(0)
        torch.manual_seed(0)
        step.optimizer.zero_grad(set_to_none=True)
        total, out = step.loss(images, masks, global_step=0, valid_samples=w)
        for k in heads:
            if k in out and out[k].requires_grad:
                out[k].retain_grad()
        total.backward()
        torch.cuda.synchronize()
        at_heads = {k: out[k].grad.clone() for k in heads if k in out and out[k].grad is not None}
        return total.detach(), out, at_heads, {n: p.grad.clone() for n, p in step.nets.named_parameters() if p.grad is not None}

    t0, _, h0, g0 = run(None)
    _, _, h0b, g0b = run(None)
    t1, _, h1, g1 = run(torch.ones(M, device=dev))
    assert torch.equal(t0, t1)
    assert h0.keys() == h1.keys() and len(h0) >= 3
    for k in h0:   # the gradients the renderer and the student loss hand to the networks: bit for bit
        assert torch.equal(h0[k], h0b[k]) and torch.equal(h0[k], h1[k]), k
    assert g0.keys() == g1.keys()
    for n in g0:   # the networks' own backward (convolutions) need not repeat its bits from call to call: where two calls
        if torch.equal(g0[n], g0b[n]):   # without weights agree, the call with all-one weights must too
            assert torch.equal(g0[n], g1[n]), n
        else:
            close(g1[n], g0[n], 1e-6, "grad " + n)
    w = torch.tensor([0.0, 1.0, 0.5, 2.0] * M, device=dev)[:M]
    total, out, _, _ = run(w)
    proj_loss, win = weighted_loss(out["pooled_masks"].double(), out["projs"].detach().double(), K, w.double())
    assert torch.equal(win.cpu(), out["min_loss"].long().cpu())
    ref = proj_loss
    if K > 1 and cfg.pose_predictor_student:
        ref = ref + student_loss(out["poses"].detach(), out["pose_student"].detach(), out["min_loss"], K,
                                 cfg.pose_predictor_student_loss_weight, w)
    close(total, ref * cfg.proj_weight, TOL, "harness weighted loss")
    assert not out["pooled_masks"].requires_grad


@pytest.mark.gpu
def test_large_weights_on_the_fused_path():
    """Weights far beyond 1 on the one-candidate fused path (its loss is summed in fixed point): a finite loss equal to the
    unfused path's and to the restatement, gradients scaled by w^2 -- no bound on the weights, like the other paths."""
    import dpc.render as R
    from oracle import dpc_oracle as O
    from test_gpu_parity import close

    S, N, G = 4, 900, 32
    cfg = O.Cfg(vox_size=G, pc_gauss_kernel_size=11)
    kern = R.smoothing_kernel(cfg, 1.1)
    pc, q, s, _, _, _ = O.synth_inputs(S, N, G, 77)
    masks = _masks(S, 2 * G, 78, True).cuda()
    w = torch.tensor([300.0, 0.0, 1.0e3, 7.0], device="cuda")
    loss, proj, win, dpc, dq, ds = _fused(R, cfg, kern, pc, q, s, masks, 1, w)     # column backward fused into the forward
    assert np.isfinite(float(loss))
    with torch.no_grad():                                                           # the unfused ray march + finalize
        loss_nf, _, _ = R.pointcloud_project_loss(cfg, pc.cuda(), q.cuda(), None, None, kern, scaling_factor=s.cuda(),
                                                  gt=masks, num_candidates=1, valid_samples=w)
    ref, _ = weighted_loss(pooled(masks.double(), 2), proj.double(), 1, w.double())
    close(loss, ref, 1e-5, "fused loss, large weights")
    close(loss_nf, ref, 1e-5, "unfused loss, large weights")
    # gradients are linear in w^2: sample 3 (w = 7) against the same call with w = 1 there
    w1 = w.clone()
    w1[3] = 1.0
    d1 = _fused(R, cfg, kern, pc, q, s, masks, 1, w1)[3]
    close(dpc[3], 49.0 * d1[3], 1e-5, "dpc scales with w^2")
    assert dpc[1].abs().max().item() == 0.0


@pytest.mark.gpu
def test_captured_step_with_weights():
    """TrainStep.capture(..., valid_samples=w): the weights are a static input of the graph like the masks; the replayed
    step follows the eager one, and a replay without weights (or weights for a step captured without them) is refused."""
    import json
    import os

    from dpc.harness import TrainStep

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    cfg = type("C", (dict,), {"__getattr__": dict.__getitem__})(json.load(open(os.path.join(golden, "f10_config.json"))))
    cfg["pc_point_dropout"] = 1.0
    g = np.load(os.path.join(golden, "f10_full_step.npz"))
    state = {k[len("state/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}
    dev = torch.device("cuda")
    images, masks = torch.from_numpy(g["images"]).to(dev), torch.from_numpy(g["masks"]).to(dev)
    M = masks.shape[0]
    w = torch.tensor([0.0, 1.0, 0.5, 2.0] * M, device=dev)[:M]

    def make(capturable):
        step = TrainStep(cfg, dev, lr=1e-3, device_dropout=True, capturable=capturable)
        step.load_reference_state(state)
        return step

    eager, captured = make(False), make(True)
    replay = captured.capture(images, masks, warmup=2, valid_samples=w)
    for _ in range(2):
        eager(images, masks, w)
    le = [float(eager(images, masks, w)) for _ in range(3)]
    lc = [float(replay(images, masks, w)) for _ in range(3)]
    assert np.allclose(le, lc, rtol=1e-4), (le, lc)
    with pytest.raises(ValueError, match="valid_samples"):
        replay(images, masks)
