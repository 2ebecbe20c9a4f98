"""Dev tool (CPU, oracle): a lane-level model of k_search's workgroup queue -- how full its waves are, and how many of the
fetch's three load rounds a wave-step executes under the old and the new lane placement (csrc/ia_search_tail.h).

The trip counts are real: `oracle.broyden(..., want_iters=True)` on the sample points of a frame (every call of the render's
deformer is one launch) and on one set of occupancy probes.  The model:
  * a workgroup owns 64 consecutive points x 13 inits; solves whose first fetch lies outside the grid never enter the queue;
    the queue is init-major / point-minor;
  * 4 waves x 64 lanes step together; before a step a wave with idle lanes pulls as many items as it has idle lanes;
  * a solve of n fetches occupies its lane for n steps;
  * a step of a wave executes round R of the fetch if a live lane sits in a slot (lane & 3) that round R serves:
    slot 0 -> round 0, slot 1 -> rounds 0 and 1, slot 2 -> rounds 1 and 2, slot 3 -> round 2.
"old": a short pull fills the idle lanes in lane order and survivors stay where they are.  "new": a short pull fills slots
0, 3, 1, 2 in that order, and a wave with at most 32 (16) live lanes moves them to slots {0, 3} ({0}).

    python tools/model_search_tail.py [--frames 0 60 150] [--res 192] > profiles/search_tail_model.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instantavatar_amd import synthetic as syn   # noqa: E402
from oracle import oracle as orc                 # noqa: E402

NP, WAVES, LANES = 64, 4, 64
SLOT_ROUNDS = np.array([0b001, 0b011, 0b110, 0b100])      # rounds (bit R) that serve slot lane & 3
SLOT = np.arange(LANES) & 3
PRIORITY = np.argsort(np.array([0, 2, 3, 1])[SLOT] * LANES + np.arange(LANES), kind="stable")   # lanes in hand-out order 0, 3, 1, 2


def tail_dest_lanes(n):
    """lanes of the class of n survivors, in rank order (ia_tail_slot_lane)"""
    r = np.arange(n)
    return 4 * (r >> 1) + 3 * (r & 1) if n > 16 else 4 * r


def run_workgroup(trips, new, acc):
    """trips: fetches of the queued solves in queue order.  acc: dict of accumulators."""
    left = np.zeros((WAVES, LANES), np.int64)             # fetches a lane's solve still needs (0: idle)
    nxt, n = 0, len(trips)
    steps = np.zeros(WAVES, np.int64)
    while True:
        for w in range(WAVES):
            idle = left[w] == 0
            k = int(idle.sum())
            if nxt < n and k:
                got = min(k, n - nxt)
                lanes = np.nonzero(idle)[0]
                if got < k and new:
                    lanes = PRIORITY[idle[PRIORITY]]
                left[w, lanes[:got]] = trips[nxt:nxt + got]
                nxt += got
            live = left[w] > 0
            a = int(live.sum())
            if a == 0:
                continue
            if new and a <= 32:
                ok = (SLOT == 0) if a <= 16 else ((SLOT == 0) | (SLOT == 3))
                if (live & ~ok).any():
                    v = left[w][live]
                    left[w] = 0
                    left[w, tail_dest_lanes(a)] = v
                    live = left[w] > 0
                    acc["moves"] += 1
            steps[w] += 1
            acc["hist"][a] += 1
            acc["lane_steps"] += a
            rounds = np.bitwise_or.reduce(SLOT_ROUNDS[SLOT[live]])
            acc["rounds"] += bin(int(rounds)).count("1")
            left[w][live] -= 1
        if nxt >= n and not left.any():
            break
    acc["wave_steps"] += int(steps.sum())
    acc["waves"] += WAVES
    acc["wg_steps"] += int(steps.max())


def queued_mask(P, world):
    """solves that enter the queue: the initial fetch has a corner inside the grid (ia_solve_is_trivial)"""
    init = world["init"]
    T = world["tfs"][list(world["bone_ids"])]
    with np.errstate(all="ignore"):
        x0 = np.einsum("nji,pnj->pni", T[:, :3, :3], P[:, None, :] - T[None, :, :3, 3])
        g = (x0 + init["offset_kernel"]) * init["scale_kernel"]
        dims = np.array([init["W"], init["H"], init["D"]])
        f0 = np.floor((g + 1) / 2 * (dims - 1))
    return ~((f0 < -1) | (f0 >= dims)).any(-1)


def model_launches(launches, world, name):
    accs = {new: dict(hist=np.zeros(LANES + 1, np.int64), lane_steps=0, rounds=0, wave_steps=0, waves=0, wg_steps=0, moves=0) for new in (False, True)}
    n_pts = 0
    for P in launches:
        P = np.ascontiguousarray(P, np.float32)
        n_pts += len(P)
        _, _, _, iters = orc.broyden(P, world["voxel_J"], world["tfs"], world["init"], world["bone_ids"], want_iters=True)
        q = queued_mask(P, world)
        for p0 in range(0, len(P), NP):
            it, qq = iters[p0:p0 + NP], q[p0:p0 + NP]
            trips = it.T[qq.T].astype(np.int64)            # init-major / point-minor
            for new in (False, True):
                run_workgroup(np.maximum(trips, 1), new, accs[new])
    print("== %s: %d launches, %d points, %d workgroups" % (name, len(launches), n_pts, accs[False]["waves"] // WAVES))
    for new in (False, True):
        a = accs[new]
        ws = max(a["wave_steps"], 1)
        h = a["hist"] / ws
        print("  %s placement: lane utilisation %.3f  steps per wave %.2f  steps of the slowest wave per workgroup %.2f" % (
            "new" if new else "old", a["lane_steps"] / (ws * LANES), a["wave_steps"] / max(a["waves"], 1), a["wg_steps"] / max(a["waves"] // WAVES, 1)))
        print("    wave-steps with <= 16 live lanes %.3f, <= 32 %.3f, 64 %.3f; histogram by 8s (1-8 .. 57-64): %s" % (
            h[1:17].sum(), h[1:33].sum(), h[64], " ".join("%.3f" % h[1 + 8 * k:9 + 8 * k].sum() for k in range(8))))
        print("    load rounds executed %d (%.3f per wave-step)%s" % (a["rounds"], a["rounds"] / ws,
              "  moves %d (%.2f per wave)" % (a["moves"], a["moves"] / max(a["waves"], 1)) if new else ""))
    o, n = accs[False], accs[True]
    print("  rounds executed: new / old = %.3f (%.1f %% fewer)" % (n["rounds"] / max(o["rounds"], 1), 100 * (1 - n["rounds"] / max(o["rounds"], 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[0, 60, 150])
    ap.add_argument("--res", type=int, default=192, help="image side of the modelled frames (the bench renders 512)")
    ap.add_argument("--probe-stride", type=int, default=1, help="model every n-th workgroup-sized run of the 64^3 probes")
    args = ap.parse_args()
    body = syn.make_body()
    init = orc.deformer_initialize(body, np.zeros(10, np.float32), syn.cano_pose("A_pose"), resolution=128, n_smooth=30)
    fp = syn.make_field(init["cano_joints"], init["bbox"])
    poses, tr = syn.procedural_pose_track(200)
    ro, rd = syn.make_camera_rays(args.res)
    jit = np.random.RandomState(0).rand(2, 64 ** 3, 3).astype(np.float32)
    print("k_search queue model, trip counts from the oracle; %d x %d frames of the procedural track" % (args.res, args.res))
    print("to reproduce (profiles/r04_search_phase_cycles.txt, frame impl0): steps per wave 12.8, lane utilisation 0.68 "
          "(9.2 M lane-steps in 13.5 M slots); probe impl0: steps per wave 2.5")
    for k, f in enumerate(args.frames):
        world = orc.make_world(body, init, fp, np.zeros(10, np.float32), poses[f, 3:], poses[f, :3], tr[f], syn.INIT_BONES)
        aabb, density, occ = orc.density_grid_initialize(world, jit, 64)
        o, d, near, far = orc.transform_rays_w2s(ro, rd, world["w2s"])
        log = []

        def model(p):
            log.append(p.copy())
            return orc.deform_query(p, world, True)
        orc.render_test(o, d, near, far, occ, aabb, model)
        model_launches(log, world, "frame %d, sample points" % f)
        if k == 0:
            G = 64
            c = np.stack(np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
            probe = (((c + jit[0]) / G) * (aabb[1] - aabb[0]) + aabb[0]).astype(np.float32)
            if args.probe_stride > 1:
                probe = probe.reshape(-1, NP, 3)[::args.probe_stride].reshape(-1, 3)
            model_launches([probe], world, "frame %d, occupancy probes (one 64^3 set%s)" % (f, ", every %d-th workgroup" % args.probe_stride if args.probe_stride > 1 else ""))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
