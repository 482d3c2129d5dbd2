"""One training step of the reference's unsupervised shape-and-pose model around dpc.render.

Follows ModelPointCloud.forward / get_loss (dpc/models/model_pc_to.py:289-336, 339-408, 410-489) and the loop body
of dpc/run/train_to.py:110-134 for the live configuration of the experiments (predict_pose, K pose candidates with a
student, learned occupancy scale, no rgb / drc losses, no translation, fixed focal length):

    images [B*V,3,S,S] -> encoder -> ids [B*V,z]; the first view's id of every object -> decoder -> points [B,N,3]
    pose FC of every image -> K candidate quaternions + 1 student quaternion per image
    points, scales repeated V*K times (candidate-minor), optional point dropout
    renderer + min-of-K silhouette loss in ONE call (dpc.render.pointcloud_project_loss), which also pools the masks and
    applies the per-view weights (valid_samples, cfg.variable_num_views)
    student loss against the winning candidate, (proj + student) * proj_weight, backward, Adam

Depth supervision (cfg.proj_depth_weight != 0, one pose candidate per image; add_proj_depth_loss, dpc/util/losses.py:113-136,
called from get_loss): the renderer's projection (dpc.render.pointcloud_project_fast), the silhouette loss and the fused
expected-depth loss (dpc.render.proj_depth_loss) on the same projection,
    total = proj_weight * (proj + student) + proj_depth_weight * depth.
With the default weight of 0 the step is the one above.

Colour supervision (cfg.pc_rgb and cfg.proj_rgb_weight != 0, one pose candidate per image; add_proj_rgb_loss,
dpc/util/losses.py:69-90): the decoder's per-point colours, replicated like the points, are projected on the same projection
(dpc.render.proj_rgb_loss) and compared with the input images,
    total = proj_weight * (proj + student) + proj_depth_weight * depth + proj_rgb_weight * rgb.
Under cfg.pc_rgb_deterministic the colour node reads the decoder's colour sets in place (no replicated all_rgb) and sums the
colour grid in fixed point: the colour terms are then the same bits on every run.

Ray-consistency terms (one pose candidate per image), further nodes on the same projection:
    cfg.drc_weight != 0: add_drc_loss (dpc/util/losses.py:49-66; get_loss, model_pc_to.py:396-397) on the pooled masks --
    add_proj_loss has replaced inputs['masks'] by them when add_drc_loss runs (:354-366) -- dpc.render.drc_loss;
    cfg.pc_rgb and cfg.drc_rgb_weight != 0: add_drc_rgb_loss (losses.py:93-110), dpc.render.drc_rgb_loss, sharing the colour
    grids with the colour loss above.  The reference defines that loss and its weight but never calls it from get_loss:
    this term is the one place where the step goes beyond get_loss.
    total += drc_weight * drc + drc_rgb_weight * drc_rgb.

Smoothed ground truth (cfg.pc_gauss_filter_gt; dpc/models/model_pc.py:398-404, dpc/util/losses.py:128-129): the masks are
resized to the silhouette's size and blurred with this step's Gaussian once per step, by one node (dpc.render.smooth_gt),
honouring cfg.pc_gauss_filter_gt_switch_off; that tensor is the ground truth of the silhouette loss (K = 1 and K candidates,
fused or as a node on the projection), of add_drc_loss, and out["pooled_masks"].  The depth maps are prepared likewise for
the depth loss, and under cfg.pc_gauss_filter_gt_rgb the images for the colour loss, with the same sigma
(model_pc_to.py:400); pc_gauss_filter_gt_rgb with drc_rgb_weight != 0 is refused.  In a captured step the node reads device
taps of the step's own (dpc.render.DeviceTaps), rewritten in front of every replay -- the identity kernel while the
switch-off holds -- so neither sigma nor the threshold needs a recapture.

cfg.pc_fast == false (compute_projection's else-branch, dpc/models/model_pc.py:249-252): the exact Gaussian renderer
dpc.render.pointcloud_project_exact with sigma = get_smooth_sigma(step) / vox_size as a launch argument, the min-of-K
silhouette loss on its projection and the student term; no occupancy scale (the reference passes none on this path).  The
depth, colour and ray-consistency losses are nodes on the fast path's grids and raise NotImplementedError naming pc_fast, and
so do capture() / capture_compute(): a captured graph freezes launch arguments, sigma among them.
"""
import numpy as np
import torch
import torch.nn.functional as F

import dpc.render as R

from .nets import StepNets


def pooled_masks(masks, size):
    """[M,1,Hm,Wm] masks -> [M,size,size,1], average-pooled like add_proj_loss (model_pc_to.py:346-356)."""
    if masks.shape[2] < size:
        raise ValueError("GT size should not be smaller than the prediction size")
    if masks.shape[2] > size:
        masks = F.avg_pool2d(masks, masks.shape[2] // size)
    return masks.permute(0, 2, 3, 1).contiguous()


def student_loss(poses, student, winner, num_candidates, weight, weights=None):
    """add_student_loss (model_pc_to.py:442-489), rotation-difference form: 1 - <teacher, student>_w^2, teachers detached;
    `weights` [S] | None: the per-view weights (valid_samples) of cfg.variable_num_views, NOT squared (:461-464, 480).

    The reference builds diff = normalise(teacher * conj(student)) and reads its w component.  That component is
    <teacher, student> / (|teacher| |student|) (the Hamilton product's norm is the product of the norms), which is what is
    computed here, in float64 like the reference: a dozen launches forward + backward instead of eighty-five."""
    teachers = poses.reshape(-1, num_candidates, 4)
    pick = winner.long().view(-1, 1, 1).expand(-1, 1, 4)
    t = teachers.gather(1, pick).squeeze(1).detach().double()
    s = student.double()
    dot = (t * s).sum(-1)
    norm2 = (t * t).sum(-1) * (s * s).sum(-1)
    term = 1.0 - dot * dot / norm2
    if weights is not None:
        term = term * weights.double()
    return term.sum() / winner.shape[0] * weight


def device_point_dropout(points, keep_prob, generator=None):
    """pc_point_dropout (point_cloud_to.py:269-295) without the host: int(N*keep) distinct random points per cloud,
    chosen on the device (dpc.render.point_dropout_indices).  Same distribution as the reference's
    np.random.choice(replace=False), different random stream.  Materialises the kept points; the
    training step below hands the INDICES to the renderer instead and keeps the point sets shared."""
    B, N = points.shape[0], points.shape[1]
    idx = R.point_dropout_indices(B, N, keep_prob, points.device, generator)
    return points.gather(1, idx.long().unsqueeze(-1).expand(B, idx.shape[1], 3))


def _copy_static(static, new):
    """Refill a captured step's static weights; a step captured without weights takes none, one captured with them needs them."""
    if (static is None) != (new is None):
        raise ValueError("valid_samples: give them at every replay exactly when the step was captured with them")
    if static is not None:
        static.copy_(new)


class TrainStep:
    def __init__(self, cfg, device, lr=1e-4, device_dropout=False, capturable=False, fused_adam=None):
        """capturable: build Adam with its step counters on the device, so that the whole step (networks, renderer, loss,
        backward, optimiser) can be captured into ONE HIP graph with capture().
        fused_adam (default: on a GPU): torch's single-kernel Adam -- the same update rule as the reference's
        torch.optim.Adam(lr, weight_decay) (train_to.py:72), one pass over the parameters instead of a dozen foreach passes
        plus, with capturable=True, six tiny kernels per parameter for the bias corrections (0.7 ms of a 3 ms step)."""
        self.cfg, self.device, self.device_dropout = cfg, device, device_dropout
        self.nets = StepNets(cfg).to(device)
        if fused_adam is None:
            fused_adam = torch.device(device).type == "cuda"
        self.optimizer = torch.optim.Adam(self.nets.parameters(), lr=lr, weight_decay=cfg.weight_decay,
                                          capturable=capturable, fused=bool(fused_adam))  # train_to.py:73-74
        self._graph = None
        self._schedule = None      # dpc.render.DeviceSchedule ONLY while a graph is being captured (record() below): an eager
                                   # loss() / __call__ on this object afterwards computes its values from the step it is asked for
        self._captured_schedule = None   # the schedule the current graph's kernels read; rewritten in front of every replay
        self._gt_taps = None       # dpc.render.DeviceTaps of the ground-truth node (cfg.pc_gauss_filter_gt), like _schedule:
                                   # set ONLY while a graph is being captured
        self._captured_gt_taps = None    # the taps the current graph's ground-truth node reads; rewritten like the schedule
        self.recaptures = 0
        self.global_step = 0
        self.grad_sync, self.sync_samples = None, (1, 1)

    def load_reference_state(self, state_dict):
        self.nets.load_state_dict(state_dict)

    def predict(self, images):
        cfg, n = self.cfg, self.nets
        enc = n.encoder(images)
        first_view = enc["ids"][::cfg.step_size]  # pool_single_view(cfg, ids, 0), model_base_to.py:8-10
        out = {"ids": enc["ids"], "scaling_factor": n.scalePred(first_view)}
        if cfg.get("pc_rgb", False):   # decoder_out['xyz'], decoder_out['rgb'] (model_pc_to.py:216-219)
            out["points_1"], out["rgb_1"] = n.decoder(first_view, enc["conv_features"][::cfg.step_size])
        else:
            out["points_1"] = n.decoder(first_view)
        out.update(n.poseNet(enc["poses"]))
        return out

    def loss(self, images, masks, global_step=None, valid_samples=None, depths=None):
        """Forward of one step; returns (total loss, dict of the pieces the reference's outputs dict would hold).
        masks [B*V,1,Hm,Wm] go to the renderer as they are (it pools them to the silhouette size inside its kernels);
        valid_samples [B*V] | None weights every view's projection and student terms (cfg.variable_num_views);
        depths [B*V,Hd,Wd,1] (inputs["depths"]) are needed, and only read, when cfg.proj_depth_weight != 0.
        With cfg.pc_rgb and cfg.proj_rgb_weight != 0 the images themselves are the colour loss's ground truth."""
        cfg = self.cfg
        depth_weight = cfg.get("proj_depth_weight", 0.0)
        rgb_weight = cfg.get("proj_rgb_weight", 0.0) if cfg.get("pc_rgb", False) else 0.0
        drc_weight = cfg.get("drc_weight", 0.0)
        drc_rgb_weight = cfg.get("drc_rgb_weight", 0.0) if cfg.get("pc_rgb", False) else 0.0
        filter_gt, filter_rgb = bool(cfg.get("pc_gauss_filter_gt", False)), bool(cfg.get("pc_gauss_filter_gt_rgb", False))
        if filter_rgb and drc_rgb_weight != 0:
            raise NotImplementedError("pc_gauss_filter_gt_rgb: true with drc_rgb_weight != 0: the reference never smooths the "
                                      "images of add_drc_rgb_loss (dpc/util/losses.py:93-110) and never calls that loss; the "
                                      "two terms would read different ground truth")
        if not cfg.get("pc_fast", True):
            for key, weight in (("proj_depth_weight", depth_weight), ("proj_rgb_weight", rgb_weight), ("drc_weight", drc_weight),
                                ("drc_rgb_weight", drc_rgb_weight)):
                if weight != 0:
                    raise NotImplementedError("%s != 0 with pc_fast: false: the supervised losses are nodes on the fast "
                                              "renderer's grids; the exact renderer returns the silhouette only" % key)
            return self._loss_exact(self.predict(images), masks, self.global_step if global_step is None else global_step, valid_samples)
        for key, weight in (("drc_weight", drc_weight), ("drc_rgb_weight", drc_rgb_weight)):
            if weight != 0 and cfg.pose_predict_num_candidates != 1:
                raise NotImplementedError("%s != 0 needs pose_predict_num_candidates == 1: with K candidates the reference's "
                                          "ray potentials do not broadcast" % key)
        if rgb_weight != 0 and cfg.pose_predict_num_candidates != 1:
            raise NotImplementedError("proj_rgb_weight != 0 needs pose_predict_num_candidates == 1: colour for K pose "
                                      "candidates is not implemented")
        if depth_weight != 0:
            if cfg.pose_predict_num_candidates != 1:
                raise NotImplementedError("proj_depth_weight != 0 needs pose_predict_num_candidates == 1: with K candidates "
                                          "the reference's depth loss does not broadcast")
            if depths is None:
                raise ValueError("proj_depth_weight != 0: the step needs `depths` (inputs['depths'], cfg.saved_depth)")
        step = self.global_step if global_step is None else global_step
        out = self.predict(images)
        K, V = cfg.pose_predict_num_candidates, cfg.step_size
        all_scales = out["scaling_factor"].repeat_interleave(V * K, dim=0) if cfg.pc_learn_occupancy_scaling else None
        all_points, point_index = out["points_1"], None  # [B,N,3] shared by the V*K clouds of an object, read in place
        sched = self._schedule       # inside a captured step: this step's sigma / keep-count live in device memory
        if cfg.pc_point_dropout != 1:                     # every replica drops its own points (:254-258 after :302-306)
            keep = R.get_dropout_prob(cfg, step)
            clouds = all_points.shape[0] * V * K
            if sched is not None:    # rows of `capacity` slots, the live count is read on the device at every replay
                point_index = R.point_dropout_indices(clouds, all_points.shape[1], (sched.capacity + 0.5) / all_points.shape[1],
                                                      all_points.device, n_live=sched.n_live)
            elif self.device_dropout:
                point_index = R.point_dropout_indices(clouds, all_points.shape[1], keep, all_points.device)
            else:  # the reference's host RNG protocol (one np.random.choice per cloud, in batch order), indices only
                n_out = int(all_points.shape[1] * keep)
                host = np.stack([np.random.choice(all_points.shape[1], n_out, replace=False) for _ in range(clouds)])
                point_index = torch.from_numpy(host.astype(np.int32)).to(all_points.device)
        kernel = R.smoothing_kernel(cfg, R.get_smooth_sigma(cfg, step))
        # cfg.pc_gauss_filter_gt: the masks are resized and smoothed once, with this step's sigma, and the same tensor feeds the
        # silhouette loss and add_drc_loss (add_proj_loss stores it back into inputs['masks'], model_pc_to.py:354-366, 396-397)
        gt_masks = self._prepared_gt(masks, "masks", step) if filter_gt else masks
        prepared = lambda on: {"gt_prepared": True} if on else {}   # without the keys the losses are called as before
        if depth_weight != 0 or rgb_weight != 0 or drc_weight != 0 or drc_rgb_weight != 0:
            # projection, silhouette loss and depth / colour / ray-consistency losses as nodes on one projection: their gradients
            # join the silhouette's at the projection's outputs (get_loss, model_pc_to.py:391-408 with losses.py:23-136)
            proj_out = R.pointcloud_project_fast(cfg, all_points, out["poses"], None, None, kernel, scaling_factor=all_scales,
                                                 point_index=point_index, schedule=sched)
            proj_loss, winner = R.silhouette_loss(proj_out["proj"], gt_masks, K, valid_samples)
            total = proj_loss.double() * cfg.proj_weight
            out.update(projs=proj_out["proj"], min_loss=winner, proj_loss=proj_loss,
                       pooled_masks=gt_masks if filter_gt else pooled_masks(masks, cfg.vox_size))
            if depth_weight != 0:
                gt_depths = self._prepared_gt(depths, "depths", step) if filter_gt else depths
                depth_loss, projs_depth = R.proj_depth_loss(cfg, proj_out, gt_depths, valid_samples, return_depth=True,
                                                            **prepared(filter_gt))   # one pass
                total = total + depth_loss.double() * depth_weight
                out.update(depth_loss=depth_loss, projs_depth=projs_depth)
            if drc_weight != 0:   # on the masks add_proj_loss pooled (model_pc_to.py:354-366), at their own size
                drc = R.drc_loss(cfg, proj_out, out["pooled_masks"], valid_samples, **prepared(filter_gt))
                total = total + drc.double() * drc_weight
                out.update(drc_loss=drc)
            if (rgb_weight != 0 or drc_rgb_weight != 0) and cfg.get("pc_rgb_deterministic", False):
                # the decoder's colour sets, read in place through the projection's own replica / dropout addressing
                all_rgb = out["rgb_1"]
                grids = R.rgb_grids(cfg, proj_out, all_rgb, kernel, point_index=point_index)
            elif rgb_weight != 0 or drc_rgb_weight != 0:
                all_rgb = R.replicate_rgb(out["rgb_1"], out["poses"].shape[0], point_index)   # model_pc_to.py:254-258, 323-329
                grids = R.rgb_grids(cfg, proj_out, all_rgb, kernel)   # one colour splat and smoothing for both colour terms
                out.update(all_rgb=all_rgb)
            if rgb_weight != 0:   # get_loss hands add_proj_rgb_loss the same sigma_rel (model_pc_to.py:400)
                gt_images = self._prepared_gt(images, "images", step) if filter_rgb else images
                rgb_loss, projs_rgb = R.proj_rgb_loss(cfg, proj_out, all_rgb, gt_images, kernel, valid_samples, return_rgb=True,
                                                      grids=grids, **prepared(filter_rgb))
                total = total + rgb_loss.double() * rgb_weight
                out.update(rgb_loss=rgb_loss, projs_rgb=projs_rgb)
            if drc_rgb_weight != 0:
                drc_rgb = R.drc_rgb_loss(cfg, proj_out, all_rgb, images, kernel, valid_samples, grids=grids)
                total = total + drc_rgb.double() * drc_rgb_weight
                out.update(drc_rgb_loss=drc_rgb)
            return total, out
        proj_loss, proj_out, winner = R.pointcloud_project_loss(cfg, all_points, out["poses"], None, None, kernel,
                                                                scaling_factor=all_scales, gt=gt_masks, num_candidates=K,
                                                                point_index=point_index, schedule=sched,
                                                                valid_samples=valid_samples)
        # for the outputs dict only: the loss above pooled the masks itself (or read the prepared ones)
        gt = gt_masks if filter_gt else pooled_masks(masks, cfg.vox_size)
        total = proj_loss.double()
        if K > 1 and cfg.pose_predictor_student:
            out["student_loss"] = student_loss(out["poses"], out["pose_student"], winner, K, cfg.pose_predictor_student_loss_weight,
                                               valid_samples)
            total = total + out["student_loss"]
        total = total * cfg.proj_weight
        out.update(projs=proj_out["proj"], min_loss=winner, proj_loss=proj_loss, pooled_masks=gt)
        return total, out

    def _loss_exact(self, out, masks, step, valid_samples):
        """The step of cfg.pc_fast == false (model_pc.py:233-252): every cloud its own copy of the points (tf_repeat_0,
        then the point dropout), pointcloud_project(cfg, all_points, poses, sigma_rel / vox_size), the projection loss."""
        cfg = self.cfg
        K, V = cfg.pose_predict_num_candidates, cfg.step_size
        all_points = out["points_1"].repeat_interleave(V * K, dim=0)
        if cfg.pc_point_dropout != 1:
            keep = R.get_dropout_prob(cfg, step)
            if self.device_dropout:
                all_points = device_point_dropout(all_points, keep)
            else:
                all_points, _ = R.pc_point_dropout(all_points, None, keep)
        sigma = R.get_smooth_sigma(cfg, step) / cfg.vox_size
        proj, _ = R.pointcloud_project_exact(cfg, all_points, out["poses"], sigma)
        filter_gt = bool(cfg.get("pc_gauss_filter_gt", False))
        gt_masks = self._prepared_gt(masks, "masks", step) if filter_gt else masks   # model_pc.py:398-404
        proj_loss, winner = R.silhouette_loss(proj, gt_masks, K, valid_samples)
        total = proj_loss.double()
        if K > 1 and cfg.pose_predictor_student:
            out["student_loss"] = student_loss(out["poses"], out["pose_student"], winner, K, cfg.pose_predictor_student_loss_weight,
                                               valid_samples)
            total = total + out["student_loss"]
        total = total * cfg.proj_weight
        out.update(projs=proj, min_loss=winner, proj_loss=proj_loss,
                   pooled_masks=gt_masks if filter_gt else pooled_masks(masks, cfg.vox_size))
        return total, out

    # ---- smoothed ground truth (cfg.pc_gauss_filter_gt, pc_gauss_filter_gt_rgb, pc_gauss_filter_gt_switch_off) ----
    def _prepared_gt(self, gt, kind, step):
        """dpc.render.smooth_gt with this step's sigma_rel: ground truth at the projection's size, [S,H,W,C].  While a graph
        is being captured the node reads the step's own device taps instead (masks only: the supervised steps are eager)."""
        if self._gt_taps is not None:
            return R.smooth_gt(self.cfg, gt, self.cfg.vox_size, kind, schedule=self._gt_taps)
        return R.smooth_gt(self.cfg, gt, self.cfg.vox_size, kind, sigma_rel=R.get_smooth_sigma(self.cfg, step))

    def _gt_tap_values(self, step):
        """The taps the captured ground-truth node applies at `step`: this step's Gaussian, or under
        cfg.pc_gauss_filter_gt_switch_off while sigma_rel < 1 the identity kernel of the same length -- multiplying finite
        values by exactly 1 and 0 returns the resized bits, so the switch follows sigma from replay to replay without a flag
        and without a recapture (tf.where(tf.less(sigma_rel, 1.0), gt, smoothed), model_pc.py:401-402)."""
        cfg = self.cfg
        sigma = R.get_smooth_sigma(cfg, step)
        taps = R.gauss_kernel_1d(int(cfg.pc_gauss_kernel_size), sigma).numpy()
        if cfg.get("pc_gauss_filter_gt_switch_off", False) and sigma < 1.0:
            taps = np.zeros_like(taps)
            taps[taps.size // 2] = 1.0
        return taps

    def _new_gt_taps(self, step):
        if not self.cfg.get("pc_gauss_filter_gt", False):
            return None
        return R.DeviceTaps(self.device, self._gt_tap_values(step))

    def __call__(self, images, masks, valid_samples=None, depths=None):
        """zero_grad, forward, loss, backward, Adam step (train_to.py:112-131).  Returns the loss tensor (no host sync).
        With `grad_sync` set (dpc.render.parallel.OverlappedGradAllReduce) the ranks' gradients are summed while the
        backward runs; `sync_samples` = (objects of this rank, objects of all ranks)."""
        if self.grad_sync is not None:
            self.grad_sync.prepare(*self.sync_samples)
        else:
            self.optimizer.zero_grad(set_to_none=True)
        total, _ = self.loss(images, masks, valid_samples=valid_samples, depths=depths)
        total.backward()
        if self.grad_sync is not None:
            self.grad_sync.finish()
        self.optimizer.step()
        self.global_step += 1
        return total.detach()

    # ---- schedules under graph replay (model_pc_to.py:59-87, 171-179, 254-258: recomputed every step) ----
    def _schedule_values(self, step):
        """(x/y taps, z taps, live points per cloud | None) of `step`."""
        cfg = self.cfg
        kern = R.smoothing_kernel(cfg, R.get_smooth_sigma(cfg, step))
        n_live = None
        if cfg.pc_point_dropout != 1:
            n_live = int(cfg.pc_num_points * R.get_dropout_prob(cfg, step))
        return kern[0].reshape(-1).numpy(), kern[2].reshape(-1).numpy(), n_live

    def _new_schedule(self, step):
        """Device-resident schedule values sized for `step` and a while after it: the tap windows of this step's sigma,
        room for half as many live points again (the keep-probability grows along the schedule)."""
        kxy, kz, n_live = self._schedule_values(step)
        capacity = None if n_live is None else min(self.cfg.pc_num_points, -(-int(n_live * 1.5) // 64) * 64)
        return R.DeviceSchedule(self.device, kxy, kz, n_live=n_live, capacity=capacity)

    def _follow_schedule(self, recapture):
        """In front of a replay: write this step's values into device memory -- or, when they no longer fit what the graph
        was captured for (sigma crossed into another tap window, the live points outgrew the rows), capture again."""
        kxy, kz, n_live = self._schedule_values(self.global_step)
        if not self._captured_schedule.tight(kxy, kz, n_live):
            recapture()
            self.recaptures += 1
        else:
            self._captured_schedule.update(kxy, kz, n_live)
            if self._captured_gt_taps is not None:   # the ground-truth node takes any values: never a reason to capture again
                self._captured_gt_taps.update(self._gt_tap_values(self.global_step))

    def _no_captured_depth_step(self):
        if not self.cfg.get("pc_fast", True):
            raise NotImplementedError("pc_fast: false: the exact renderer takes sigma as a launch argument, which a captured "
                                      "graph would freeze; the step is eager only")
        if self.cfg.get("proj_depth_weight", 0.0) != 0:
            raise NotImplementedError("proj_depth_weight != 0: the depth-supervised step is eager only (no graph capture)")
        if self.cfg.get("pc_rgb", False) and self.cfg.get("proj_rgb_weight", 0.0) != 0:
            raise NotImplementedError("proj_rgb_weight != 0: the colour-supervised step is eager only (no graph capture)")
        if self.cfg.get("drc_weight", 0.0) != 0:
            raise NotImplementedError("drc_weight != 0: the step with the ray-consistency loss is eager only (no graph capture)")
        if self.cfg.get("pc_rgb", False) and self.cfg.get("drc_rgb_weight", 0.0) != 0:
            raise NotImplementedError("drc_rgb_weight != 0: the step with the ray-consistency colour loss is eager only "
                                      "(no graph capture)")

    def capture_compute(self, images, masks, warmup=2, valid_samples=None):
        """The multi-rank variant of capture(): forward, loss and backward as ONE HIP graph whose backward accumulates
        straight into the flat buckets of `grad_sync` (every .grad is a view into them); the gradient exchange and Adam run
        eagerly after each replay (OverlappedGradAllReduce.reduce_now -- collectives are not captured).  The eager step
        hides the exchange under a launch-bound 4 ms backward; this one has a 2 ms step and exposes the exchange.
        `warmup` eager steps run first: the first one fixes which parameters take part in the exchange.
        Returns replay(images, masks[, valid_samples]) -> loss tensor (valid_samples: a static input like the masks, given
        at every replay when the capture had it)."""
        self._no_captured_depth_step()
        sync = self.grad_sync
        if sync is None:
            raise RuntimeError("capture_compute() is the step with a gradient exchange (set grad_sync); use capture() without")
        if self.cfg.pc_point_dropout != 1 and not self.device_dropout:
            raise RuntimeError("the reference's host-RNG point dropout uploads indices every step: not capturable; "
                               "use device_dropout=True")
        static_images, static_masks = images.clone(), masks.clone()
        static_valid = None if valid_samples is None else valid_samples.clone()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                self(static_images, static_masks, static_valid)
        torch.cuda.current_stream(self.device).wait_stream(side)
        for p in sync.params:                 # what finish() left: views into the buckets
            p.grad = sync.views[id(p)]
        state = {}

        def record():
            self._captured_schedule = self._schedule = self._new_schedule(self.global_step)
            self._captured_gt_taps = self._gt_taps = self._new_gt_taps(self.global_step)
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    for flat in sync.flat:
                        flat.zero_()
                    total, _ = self.loss(static_images, static_masks, valid_samples=static_valid)
                    total.backward()              # the hooks are disarmed: gradients simply land in the buckets
            finally:
                self._schedule = self._gt_taps = None   # the captured kernels keep the pointers; eager calls do not see them
            self._graph, state["graph"], state["loss"] = graph, graph, total.detach()

        record()

        def replay(new_images, new_masks, new_valid_samples=None):
            static_images.copy_(new_images)
            static_masks.copy_(new_masks)
            _copy_static(static_valid, new_valid_samples)
            self._follow_schedule(record)
            state["graph"].replay()
            sync.reduce_now(*self.sync_samples)
            self.optimizer.step()
            self.global_step += 1
            return state["loss"]

        return replay

    def capture(self, images, masks, warmup=3, valid_samples=None):
        """Capture forward + loss + backward + Adam into one HIP graph (the standard whole-step recipe of
        torch.cuda.graphs: warm up on a side stream, capture with gradients set to None, replay on static inputs).

        Everything inside the step is capture-safe: the renderer enqueues on the capturing stream and never synchronises,
        allocates through torch's (graph-private) pool, draws the point dropout on the device, and the optimiser was built
        with capturable=True.  The schedules stay step-exact: the Gaussian's tap values and the number of kept points live in
        device memory (dpc.render.DeviceSchedule) and are rewritten by one tiny launch in front of every replay from
        get_smooth_sigma / get_dropout_prob of the CURRENT global_step, like the reference recomputes them every step
        (model_pc_to.py:59-87, 171-179, 254-258); the graph is captured again, automatically, only when sigma crosses into
        another compiled tap window or the kept points outgrow the captured rows (`recaptures` counts).  Returns
        replay(images, masks[, valid_samples]) -> loss tensor (static memory, overwritten by the next replay); valid_samples
        is a static input like the masks, given at every replay when the capture had it."""
        self._no_captured_depth_step()
        if self.grad_sync is not None:
            raise RuntimeError("capture() covers the single-process step; the overlapped gradient exchange runs eagerly")
        if self.cfg.pc_point_dropout != 1 and not self.device_dropout:
            raise RuntimeError("the reference's host-RNG point dropout uploads indices every step: not capturable; "
                               "use device_dropout=True")
        if not all(g["capturable"] for g in self.optimizer.param_groups):
            raise RuntimeError("build the TrainStep with capturable=True")
        static_images, static_masks = images.clone(), masks.clone()
        static_valid = None if valid_samples is None else valid_samples.clone()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):          # lazy initialisations (Adam state, allocator, kernel attributes) happen here
                self(static_images, static_masks, static_valid)
        torch.cuda.current_stream(self.device).wait_stream(side)
        state = {}

        def record():
            self._captured_schedule = self._schedule = self._new_schedule(self.global_step)
            self._captured_gt_taps = self._gt_taps = self._new_gt_taps(self.global_step)
            self.optimizer.zero_grad(set_to_none=True)
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    total, _ = self.loss(static_images, static_masks, valid_samples=static_valid)
                    total.backward()
                    self.optimizer.step()
            finally:
                self._schedule = self._gt_taps = None   # the captured kernels keep the pointers; eager calls do not see them
            self._graph, state["graph"], state["loss"] = graph, graph, total.detach()

        record()

        def replay(new_images, new_masks, new_valid_samples=None):
            static_images.copy_(new_images)
            static_masks.copy_(new_masks)
            _copy_static(static_valid, new_valid_samples)
            self._follow_schedule(record)
            state["graph"].replay()
            self.global_step += 1
            return state["loss"]

        return replay
