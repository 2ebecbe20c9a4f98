"""Wall time of one keypoint-refinement step (loss, gradient, Adam) at F frames of the synthetic body with blend shapes: the HIP
kernels (`KeypointRefiner`: ia_kp_loss_fwd + ia_kp_loss_bwd + ia_adam_step) against the route the reference takes -- SMPL.forward
in torch ops, the loss of refine-smpl.py:187-208 under autograd, torch.optim.Adam -- on the same GPU and the same inputs.  Each
figure is the median over `--repeat` windows of `--steps` steps, every window closed by a device synchronisation, after a warm-up
window; the two routes alternate.  The loss and the gradients of the two routes are compared first.

    python tools/time_keypoints.py --frames 300 --out profiles/keypoint_refine_timing.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import synthetic
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.keypoints import BODY25_TO_POINT, MIDHIP, SMPL_KP_VERTEX, KeypointRefiner
    from instantavatar_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    F = args.frames
    body = SMPL.from_dict(synthetic.make_body(blendshapes=True)).to(dev)
    V = int(body.v_template.shape[0])
    pose_np, transl_np = synthetic.procedural_pose_track(F)
    rs = np.random.RandomState(0)
    proj = torch.tensor([[1000.0, 0, 256.0, 0], [0, 1000.0, 256.0, 0], [0, 0, 1.0, 0]], device=dev)
    betas0 = torch.tensor(rs.randn(10) * 0.3, dtype=torch.float32, device=dev)
    pose_true, transl_true = torch.tensor(pose_np, device=dev), torch.tensor(transl_np, device=dev)
    sel = torch.tensor([k for k in range(25) if k != MIDHIP], device=dev)
    mapping = torch.tensor(BODY25_TO_POINT, device=dev)
    kpv = torch.tensor(SMPL_KP_VERTEX, device=dev)

    def torch_loss(betas, pose, transl, kp, thr):
        out = body(betas=betas[None], body_pose=pose[:, 3:], global_orient=pose[:, :3], transl=transl)
        pts = torch.cat([out.joints, out.vertices[:, kpv]], 1)[:, mapping]
        p = torch.einsum("ij,mnj->mni", proj[:3, :3], pts) + proj[:3, 3]
        uv = p[..., :2] / p[..., 2:3]
        err = (kp[..., :2] - uv).square().sum(-1).sqrt() * (kp[..., 2] > thr).float()
        reg = (out.vertices[1:] - out.vertices[:-1]).square().sum(-1).sqrt()
        return err[:, sel].mean() + reg.mean(), uv

    with torch.no_grad():
        _, uv = torch_loss(betas0, pose_true, transl_true, torch.zeros((F, 25, 3), device=dev), 0.2)
    kp = torch.cat([uv + torch.tensor(rs.randn(F, 25, 2), dtype=torch.float32, device=dev), torch.tensor(rs.rand(F, 25, 1), dtype=torch.float32, device=dev)], -1)
    pose0 = pose_true + 0.03 * torch.tensor(rs.randn(F, 72), dtype=torch.float32, device=dev)
    transl0 = transl_true + 0.02 * torch.tensor(rs.randn(F, 3), dtype=torch.float32, device=dev)
    thr = 0.2
    r = KeypointRefiner(body, proj, kp, threshold=thr)

    # the two routes compute the same thing
    leaves = [x.clone().requires_grad_(True) for x in (betas0, pose0, transl0)]
    L, _ = torch_loss(*leaves, kp, thr)
    L.backward()
    out, g = r.loss_and_grad(betas0, pose0, transl0)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    agree = "loss %.6f (HIP) / %.6f (torch); largest gradient difference over largest entry: betas %.1e, pose %.1e, transl %.1e" % (
        float(out["loss"]), float(L), rel(g["betas"], leaves[0].grad), rel(g["pose"], leaves[1].grad), rel(g["transl"], leaves[2].grad))

    hp = [torch.nn.Parameter(x.clone()) for x in (betas0, pose0, transl0)]
    for x in hp:
        x.grad = torch.empty_like(x)
    hopt = FusedAdam(hp, lr=1e-3)
    hloss = torch.empty(3, device=dev)

    def hip_step():
        r._fwd(hp[0].data, hp[1].data, hp[2].data, hloss)
        r._bwd(hp[0].data, hp[1].data, hp[2].data, hp[0].grad, hp[1].grad, hp[2].grad)
        hopt.step()

    def hip_grad():
        r._fwd(hp[0].data, hp[1].data, hp[2].data, hloss)
        r._bwd(hp[0].data, hp[1].data, hp[2].data, hp[0].grad, hp[1].grad, hp[2].grad)

    tp = [torch.nn.Parameter(x.clone()) for x in (betas0, pose0, transl0)]
    topt = torch.optim.Adam(tp, lr=1e-3)

    def torch_step():
        topt.zero_grad()
        loss, _ = torch_loss(*tp, kp, thr)
        loss.backward()
        topt.step()

    def torch_grad():
        for x in tp:
            x.grad = None
        loss, _ = torch_loss(*tp, kp, thr)
        loss.backward()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps

    routes = [("HIP   loss + gradient + Adam", hip_step), ("torch loss + gradient + Adam", torch_step),
              ("HIP   loss + gradient", hip_grad), ("torch loss + gradient", torch_grad)]
    for _, fn in routes:
        window(fn)
    times = {name: [] for name, _ in routes}
    for _ in range(args.repeat):
        for name, fn in routes:
            times[name].append(window(fn))
    lines = ["one keypoint-refinement step at F = %d frames, V = %d (synthetic body with blend shapes) on %s" % (F, V, torch.cuda.get_device_name(0)),
             "wall time per step in ms: median (min .. max) of %d windows of %d steps, each closed by a device synchronisation, after a warm-up window"
             % (args.repeat, args.steps)]
    for name, _ in routes:
        t = times[name]
        lines.append("  %-30s %9.3f  (%.3f .. %.3f)" % (name, statistics.median(t), min(t), max(t)))
    lines.append("HIP = ia_kp_loss_fwd + ia_kp_loss_bwd (+ ia_adam_step); torch = SMPL.forward in torch ops + refine-smpl.py's loss under autograd (+ torch.optim.Adam)")
    lines.append("agreement before timing: " + agree)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
