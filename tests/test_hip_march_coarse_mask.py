"""The training marcher with the coarse occupancy mask computes what it computes without it, bit for bit (GPU).

* pvd_occ_coarse_mask against the numpy build of tests/coarse_mask_ref.py, on every grid of the CPU test
  (tests/test_march_coarse_mask.py).
* pvd_march_rays_train_mask with the mask against the same call with NULL: rays, counter, xyzs, dirs, deltas and the chunk records
  of the rays that sample, torch.equal, for N = 257 rays (a partial last workgroup), max_steps 1024 and 8 (the cap binds), perturb
  on and off, bound 1 and 2.  Once more with the CPU test's 2000 rays on the grids where the mask acts most: the device's 64-point
  test is pinned by this on/off equality alone (the numpy restatement the CPU test proves conservative is not compared lane by lane).
* a model's mask follows its bitfield through every writer: install_occupancy's copy_, load_state_dict, update_extra_state, a write
  through data_ptr() announced by note_occupancy_changed() (the tail of RayDP.sync_occupancy) and a copy_ nobody announced (caught
  by the key on the bitfield's version).  RayDP.sync_occupancy itself needs more than one rank and is not run here: what it does to
  the mask is its closing note_occupancy_changed() (pvd/ray_dp.py), which the announced raw write stands in for.  Each starts from a mask that would call the new grid's rays empty, so a stale mask fails."""
import numpy as np
import pytest
import torch

import coarse_mask_ref as ref

pytestmark = pytest.mark.gpu

H, N = 128, 257


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _march(dev, o, d, bits, nears, fars, bound, C, max_steps, perturb, mask):
    import pvd_hip
    N = o.shape[0]
    M = N * max_steps + 1
    xyzs, dirs, deltas = (torch.zeros(M, k, device=dev) for k in (3, 3, 2))
    rays = torch.zeros(N, 3, dtype=torch.int32, device=dev)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    pvd_hip.march_rays_train(o, d, bits, bound, 0.0, max_steps, N, C, H, M, nears, fars, xyzs, dirs, deltas, rays, counter, perturb,
                             coarse_mask=mask)
    rec = pvd_hip._march_workspace(dev, N).clone().cpu().numpy()[:N * 256].reshape(N, 256)  # MarchRayRecords, csrc/raymarching.hip
    return dict(rays=rays, counter=counter, xyzs=xyzs, dirs=dirs, deltas=deltas), rec


def _records_equal(a, b, counts):
    """{n, overflow, pad[2]; 15 x {mask u64, t_base f32, pad u32}} per ray: n, overflow and the first n chunks' mask and t_base."""
    for n in np.flatnonzero(counts > 0):
        ha, hb = a[n, :8].view(np.uint32), b[n, :8].view(np.uint32)
        if not np.array_equal(ha, hb):
            return False
        ca, cb = a[n, 16:16 + 16 * ha[0]].reshape(-1, 16)[:, :12], b[n, 16:16 + 16 * ha[0]].reshape(-1, 16)[:, :12]
        if not np.array_equal(ca, cb):
            return False
    return True


@pytest.fixture(scope="module", params=[1.0, 2.0], ids=["bound1", "bound2"])
def grids(request):
    bound = request.param
    C = 1 + int(np.ceil(np.log2(bound)))
    return bound, C, ref.grids(C, H, seed=int(bound))


MANY = ("random1", "random5", "blocky_aligned", "blocky_odd", "empty", "cell_127_63_0", "cell_63_63_127")


@pytest.mark.parametrize("n_rays,max_steps_set,names", [(N, (1024, 8), None), (2000, (1024,), MANY)], ids=["257rays", "2000rays"])
def test_mask_kernel_matches_numpy_and_the_march_is_unchanged(dev, grids, n_rays, max_steps_set, names, capsys):
    import pvd_hip
    import raymarching as rm
    bound, C, all_grids = grids
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, device=dev)
    skipped = walked = 0
    for name, dense in all_grids.items():
        if names is not None and name not in names:
            continue
        bits_np = ref.bitfield_of(dense)
        bits = torch.from_numpy(bits_np).to(dev)
        mask = torch.full((pvd_hip.coarse_mask_bytes(C, H),), 7, dtype=torch.uint8, device=dev)
        pvd_hip.occ_coarse_mask(bits, C, H, mask)
        assert np.array_equal(mask.cpu().numpy(), ref.coarse_mask(bits_np, C, H)), name
        o_np, d_np = ref.rays(n_rays, bound, dense, seed=len(name))
        o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
        nears, fars = rm.near_far_from_aabb(o, d, aabb, 0.2)
        for max_steps in max_steps_set:
            for perturb in (True, False):
                off, rec_off = _march(dev, o, d, bits, nears, fars, bound, C, max_steps, perturb, None)
                on, rec_on = _march(dev, o, d, bits, nears, fars, bound, C, max_steps, perturb, mask)
                for k in off:
                    assert torch.equal(on[k], off[k]), (name, max_steps, perturb, k)
                counts = off["rays"][:, 2].cpu().numpy()
                assert _records_equal(rec_on, rec_off, counts), (name, max_steps, perturb)
                walked += int((counts > 0).sum())
                skipped += int((counts == 0).sum())
    with capsys.disabled():
        print("\nbound %g, %d rays: %d marches of rays that sample, %d of rays that do not" % (bound, n_rays, walked, skipped))


def test_the_models_mask_follows_every_writer_of_the_bitfield(dev):
    import pvd_hip
    from pvd.config import PVDConfig
    from pvd.ops import hip_ops
    from pvd.scene import ChairScene
    from pvd.workload import install_occupancy, make_model
    torch.manual_seed(0)
    opt = PVDConfig(num_rays=N)
    ops = hip_ops()
    rm = ops.raymarching
    model = make_model(ops, opt, "hash", True, dev)
    model.train()
    dense = np.ones((model.cascade, H, H, H), bool)
    o_np, d_np = ref.rays(N, opt.bound, dense, seed=3)
    o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)

    def agree(what, want_samples):
        """model.march (takes the model's mask) against the plain operator without one."""
        assert model.coarse_mask() is not None
        (xyzs, dirs, deltas, rays), (nears, fars) = model.march(o, d, perturb=True, force_all_rays=True)
        x0, d0, l0, r0 = rm.march_rays_train(o, d, model.bound, model.density_bitfield, model.cascade, model.grid_size, nears, fars,
                                             None, -1, True, 128, True, 0, 1024)
        assert torch.equal(rays, r0) and torch.equal(xyzs, x0) and torch.equal(dirs, d0) and torch.equal(deltas, l0), what
        total = int(r0[:, 2].sum())
        assert (total > 0) == want_samples, (what, total)
        want = ref.coarse_mask(model.density_bitfield.cpu().numpy(), model.cascade, H)
        assert np.array_equal(model.density_coarse_mask.cpu().numpy(), want), what

    def empty_it():
        model.density_bitfield.zero_()
        model.note_occupancy_changed()
        agree("emptied", False)
        assert int(model.density_coarse_mask.sum()) == 0

    ptr = model.density_coarse_mask.data_ptr()
    empty_it()
    install_occupancy(model, ChairScene(), opt)            # DistillWorkload's analytic grid: copy_ + note_occupancy_changed
    agree("install_occupancy", True)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    assert "density_coarse_mask" not in state              # derived state is not saved
    empty_it()
    model.load_state_dict(state)                           # a checkpoint load
    agree("load_state_dict", True)
    empty_it()
    model.density_grid.copy_(torch.rand_like(model.density_grid))  # the threshold is the mean: about half the cells pass
    model.update_extra_state()                             # packbits on the device, through data_ptr()
    agree("update_extra_state", True)
    empty_it()
    full = torch.full_like(model.density_bitfield, 255)
    pvd_hip.packbits(torch.ones(model.cascade * H ** 3, device=dev), model.density_bitfield.numel(), 0.5, model.density_bitfield)
    assert torch.equal(model.density_bitfield, full)
    model.note_occupancy_changed()                         # a raw write, announced (RayDP.sync_occupancy ends the same way)
    agree("raw write + note_occupancy_changed", True)
    empty_it()
    model.density_bitfield.copy_(full)                     # a writer nobody announced: the key on the tensor's version catches it
    agree("unannounced copy_", True)
    assert model.density_coarse_mask.data_ptr() == ptr     # rebuilt in place throughout: recorded graphs keep their address
