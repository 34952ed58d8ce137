"""Training batches made on the device from a resident uint8 image stack: the data side of a teacher step (NeRFDataset.collate,
distill_mutual/provider.py:278-308 -> get_rays, distill_mutual/utils.py:324-404; the random background and alpha blend of
train_step, utils.py:987-995; the --error_map feedback, utils.py:1120-1129) as one or two launches per batch (pvd_image_batch) and
one for the feedback (pvd_error_map_update).  Nothing here synchronises with the host, so `fill` and `feedback` can be recorded
into TeacherTrainer's 16-step graph (capture_block(batches, source)); a replay then trains on 16 fresh batches.

    src = DeviceBatcher.from_scene(scene, aabb, min_near, num_rays=4096, seed=0, error_map=True)
    batches = [src.new_batch() for _ in range(16)]
    src.fill(batches[0]); loss, pred = trainer.train_step(*batches[0]); src.feedback(batches[0], pred)     # eager
    trainer.capture_block(batches, src); trainer.train_block()                                              # 16 steps per launch
"""
import torch


class Batch(tuple):
    """(rays_o, rays_d, gt, bg) [1,N,3] -- what TeacherTrainer takes -- with the slot's private buffers as attributes:
    inds, inds_coarse int64 [N], view int32 [1], nears, fars [N]."""

    def __new__(cls, rays_o, rays_d, gt, bg, **private):
        self = super().__new__(cls, (rays_o, rays_d, gt, bg))
        self.__dict__.update(private)
        return self


class DeviceBatcher:
    def __init__(self, images_u8, poses, intrinsics, aabb, min_near, num_rays, seed, error_map=False, grid=128):
        """images_u8 [V,H,W,3|4] uint8 and poses [V,4,4] f32 on the device; intrinsics (fx, fy, cx, cy); aabb [6].
        error_map=True: pixels are drawn by a per-view error map on a grid x grid lattice (all ones to begin with,
        provider.py:232-237) that `feedback` updates; otherwise uniformly."""
        import pvd_hip
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] not in (3, 4):
            raise ValueError("images_u8 must be a uint8 [V,H,W,3|4] stack")
        if not images_u8.is_cuda:
            raise ValueError("the image stack must be resident on the device")
        if error_map and not 0 < int(grid) <= pvd_hip.DATA_MAX_GRID:
            raise ValueError("grid must be in 1..%d" % pvd_hip.DATA_MAX_GRID)
        if error_map and num_rays > int(grid) ** 2:
            raise ValueError("an error map of %d cells cannot give %d distinct cells" % (int(grid) ** 2, num_rays))
        dev = images_u8.device
        self.device = dev
        self.images = images_u8.contiguous()
        self.V, self.H, self.W, self.C = (int(v) for v in self.images.shape)
        self.poses = poses.to(dev, torch.float32).contiguous()
        assert self.poses.shape == (self.V, 4, 4)
        self.intrinsics = tuple(float(v) for v in intrinsics)
        self.aabb = torch.as_tensor(aabb, dtype=torch.float32).reshape(-1)[:6].to(dev).contiguous()
        self.min_near, self.num_rays, self.seed, self.grid = float(min_near), int(num_rays), int(seed), int(grid)
        self.state = torch.zeros(3, dtype=torch.int64, device=dev)  # {position in order, batch counter, scratch}
        self.order = torch.arange(self.V, dtype=torch.int32, device=dev)
        self.error_map = torch.ones(self.V, self.grid * self.grid, dtype=torch.float32, device=dev) if error_map else None

    @classmethod
    def from_scene(cls, scene, aabb, min_near, num_rays=None, seed=0, error_map=False, grid=128, device=None):
        """From a BlenderScene: its float images go back to the bytes they were read from ((x * 255).round() is exact for
        uint8 / 255.0 in float32 and in float16)."""
        dev = torch.device(device) if device is not None else scene.device
        u8 = (scene.images.to(dev).float() * 255.0).round().to(torch.uint8)
        return cls(u8, scene.poses, scene.intrinsics, aabb, min_near, scene.num_rays if num_rays is None else num_rays, seed,
                   error_map=error_map, grid=grid)

    def new_batch(self):
        """A static slot: (rays_o, rays_d, gt, bg) [1,N,3] with private inds / inds_coarse / view / nears / fars.
        RGB images train against white (training_target): bg is then a constant the kernel never writes."""
        N, dev = self.num_rays, self.device
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        bg = f(1, N, 3) if self.C == 4 else torch.ones(1, N, 3, dtype=torch.float32, device=dev)
        return Batch(f(1, N, 3), f(1, N, 3), f(1, N, 3), bg,
                     inds=torch.zeros(N, dtype=torch.int64, device=dev),
                     inds_coarse=torch.zeros(N, dtype=torch.int64, device=dev) if self.error_map is not None else None,
                     view=torch.zeros(1, dtype=torch.int32, device=dev), nears=f(N), fars=f(N))

    def fill(self, batch, keys_out=None):
        """The next batch into `batch` (pvd_image_batch on the current stream; no host sync; capturable)."""
        import pvd_hip
        fx, fy, cx, cy = self.intrinsics
        pvd_hip.image_batch(self.images, self.poses, self.order, self.state, self.seed, fx, fy, cx, cy, self.num_rays, self.aabb,
                            self.min_near, self.error_map, batch.view, batch.inds, batch.inds_coarse, batch[0], batch[1], batch[2],
                            batch[3] if self.C == 4 else None, batch.nears, batch.fars, keys_out)
        return batch

    def feedback(self, batch, pred):
        """The per-ray error of `pred` [.., N, 3] against the batch's ground truth into the cells the batch was drawn from
        (pvd_error_map_update); nothing without an error map."""
        if self.error_map is None:
            return
        import pvd_hip
        pred = pred.detach()
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        pvd_hip.error_map_update(self.error_map, batch.view, batch.inds_coarse, pred, batch[2], self.num_rays)

    def shuffle(self, generator=None):
        """A new random order of the views (the loader's shuffle), drawn on the device."""
        self.order.copy_(torch.randperm(self.V, device=self.device, generator=generator).to(torch.int32))
