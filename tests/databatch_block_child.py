"""Child process of tests/test_hip_databatch.py: a hash teacher trained from a DeviceBatcher, one eager block, then
capture_block(batches, source) and two train_block() calls, once without the error map (steps recorded back to back) and once
with it (next step's draw and march on the forked stream).  Everything the parent compares goes to the .npz named on the command
line.  Not collected by pytest."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "aaai2023-pvd_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

import pvd_hip  # noqa: F401  (before torch touches the device)
import torch

DEV = "cuda:0"
V, H, W, N, GRID, SEED = 17, 32, 32, 1024, 64, 4242  # 17 views: no view comes twice inside a 16-step block


def run(error_map, forked):
    from pvd.batcher import DeviceBatcher
    from pvd.config import PVDConfig
    from pvd.ops import hip_ops
    from pvd.scene import BLENDER_INTRINSICS
    from pvd.trainer import TeacherTrainer
    from pvd.workload import DistillWorkload, measure_mean_count
    os.environ["PVD_FORKED_GRAPHS"] = "1" if forked else "0"
    torch.manual_seed(0)
    opt = PVDConfig(num_rays=N, fp16=True)
    w = DistillWorkload(hip_ops(), torch.device(DEV), opt, teacher_pretrain_steps=0, seed=0)
    topt = PVDConfig(**{**opt.__dict__, "model_type": opt.teacher_type, "iters": 3000, "stage_iters": {"stage1": -1, "stage2": -1}})
    tea = w.tea
    tea.teacher_variant = True
    tea.requires_grad_(True).train()
    tea.args = tea.opt = topt
    tr = TeacherTrainer(topt, tea, torch.device(DEV), fp16=True)
    tea.mean_count = measure_mean_count(tea, w.poses, opt, generator=w.gen)

    rng = np.random.RandomState(3)
    images = rng.randint(0, 256, size=(V, H, W, 4)).astype(np.uint8)
    images[..., 3][rng.rand(V, H, W) < 0.25] = 0
    images[..., 3][rng.rand(V, H, W) < 0.25] = 255
    order = rng.permutation(V).astype(np.int32)
    intr = tuple(v * H / 800.0 for v in BLENDER_INTRINSICS)
    src = DeviceBatcher(torch.from_numpy(images).to(DEV), w.poses[:V], intr, tea.aabb_train, 0.2, N, SEED, error_map=error_map, grid=GRID)
    src.order.copy_(torch.from_numpy(order).to(DEV))
    batches = [src.new_batch() for _ in range(16)]

    drawn = np.zeros((V, GRID * GRID), bool)

    def note_cells(bs):
        if error_map:
            for b in bs:
                drawn[int(b.view[0]), b.inds_coarse.cpu().numpy()] = True
    losses = []
    for it in range(16):
        src.fill(batches[it])
        loss, pred = tr.train_step(*batches[it])
        src.feedback(batches[it], pred)
        losses.append(float(loss))
        note_cells(batches[it:it + 1])
    state_eager = src.state.cpu().numpy()
    tr.capture_block(batches, src)
    assert tr.pipelined_block == forked, "the block was not recorded in the schedule this run is about"
    state_captured = src.state.cpu().numpy()  # a recording runs nothing
    loss, pred = tr.train_block()
    losses.append(float(loss))
    note_cells(batches)
    map_before = src.error_map.cpu().numpy() if error_map else np.zeros(0, np.float32)
    loss, pred = tr.train_block()
    losses.append(float(loss))
    note_cells(batches)
    torch.cuda.synchronize()
    out = {"images": images, "order": order, "losses": np.array(losses), "state_eager": state_eager, "state_captured": state_captured,
           "state": src.state.cpu().numpy(), "pred": pred.detach().float().reshape(-1, 3).cpu().numpy(), "drawn": drawn,
           "map_before": map_before, "map": src.error_map.cpu().numpy() if error_map else np.zeros(0, np.float32),
           "global_step": np.array(tr.global_step)}
    for k, b in enumerate(batches):
        out["view%d" % k] = b.view.cpu().numpy()
        out["inds%d" % k] = b.inds.cpu().numpy()
        out["gt%d" % k] = b[2].reshape(-1, 3).cpu().numpy()
        out["bg%d" % k] = b[3].reshape(-1, 3).cpu().numpy()
        if error_map:
            out["cells%d" % k] = b.inds_coarse.cpu().numpy()
    return out


if __name__ == "__main__":
    res = {}
    for name, error_map, forked in (("uniform", False, False), ("errmap", True, True)):
        for k, v in run(error_map, forked).items():
            res["%s_%s" % (name, k)] = v
    np.savez(sys.argv[1], **res)
    print("child ok")
