"""write_png / read_png and write_obj / read_obj of pvd/mesh.py: the files a textured export consists of.  No GPU."""
import os

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("H,W", ((1, 1), (5, 7), (64, 48)))
def test_png_round_trip(H, W, tmp_path, hip_lib_built):
    from pvd.mesh import read_png, write_png
    rng = np.random.RandomState(H * 100 + W)
    img = rng.rand(H, W, 3).astype(np.float32)
    img.reshape(-1)[:3] = (0.0, 1.0, 0.5)
    if H * W > 4:
        img[1, 1] = (-0.5, 1.5, np.nan)  # clamped; NaN is 0
    path = str(tmp_path / "t.png")
    assert write_png(path, torch.from_numpy(img)) == path
    want = np.rint(np.clip(np.nan_to_num(img, nan=0.0), 0, 1) * 255).astype(np.uint8)
    back = read_png(path)
    assert back.dtype == torch.float32 and tuple(back.shape) == (H, W, 3)
    assert np.array_equal(np.rint(back.numpy() * 255).astype(np.uint8), want)
    assert np.array_equal(back.numpy(), want.astype(np.float32) / np.float32(255))
    # bytes in, the same bytes out; and what was read writes the same file again
    write_png(str(tmp_path / "u.png"), want)
    assert open(str(tmp_path / "u.png"), "rb").read() == open(path, "rb").read()
    write_png(str(tmp_path / "w.png"), back)
    assert open(str(tmp_path / "w.png"), "rb").read() == open(path, "rb").read()


@pytest.mark.parametrize("H,W", ((1, 1), (5, 7), (64, 48)))
def test_png_is_decoded_by_pil_to_the_same_bytes(H, W, tmp_path, hip_lib_built):
    Image = pytest.importorskip("PIL.Image")
    from pvd.mesh import write_png
    want = np.random.RandomState(H + W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    path = write_png(str(tmp_path / "t.png"), want)
    with Image.open(path) as im:
        assert im.mode == "RGB" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), want)


def test_read_png_refuses_what_write_png_does_not_write(tmp_path, hip_lib_built):
    from pvd.mesh import read_png, write_png
    path = str(tmp_path / "t.png")
    write_png(path, np.zeros((2, 3, 3), np.float32))
    data = open(path, "rb").read()
    open(path, "wb").write(data[:40] + bytes([data[40] ^ 1]) + data[41:])
    with pytest.raises(ValueError):
        read_png(path)
    open(path, "wb").write(b"not a png")
    with pytest.raises(ValueError):
        read_png(path)
    with pytest.raises(ValueError):
        write_png(path, np.zeros((2, 3), np.float32))


@pytest.mark.parametrize("with_normals", (False, True))
def test_obj_round_trip(with_normals, tmp_path, hip_lib_built):
    from pvd.mesh import read_obj, texture_uv, write_obj
    rng = np.random.RandomState(3)
    V, T, S = 11, 7, 8
    v = rng.randn(V, 3).astype(np.float32)
    v[0] = (0.1, 1e-20, -3e7)
    t = rng.randint(0, V, (T, 3)).astype(np.int32)
    n = rng.randn(V, 3).astype(np.float32) if with_normals else None
    uv = texture_uv(T, S)
    path = str(tmp_path / "mesh.obj")
    assert write_obj(path, torch.from_numpy(v), torch.from_numpy(t), uv, "mesh.png", normals=None if n is None else torch.from_numpy(n)) == path
    mtl = open(str(tmp_path / "mesh.mtl")).read()
    assert "newmtl material0" in mtl and "map_Kd mesh.png" in mtl.splitlines()
    text = open(path).read().splitlines()
    assert text[0] == "mtllib mesh.mtl" and "usemtl material0" in text
    assert sum(ln.startswith("v ") for ln in text) == V and sum(ln.startswith("vt ") for ln in text) == 3 * T
    assert sum(ln.startswith("vn ") for ln in text) == (V if with_normals else 0) and sum(ln.startswith("f ") for ln in text) == T
    a, b, c = (int(x) + 1 for x in t[0])
    assert ("f %d/1/%d %d/2/%d %d/3/%d" % (a, a, b, b, c, c) if with_normals else "f %d/1 %d/2 %d/3" % (a, b, c)) in text
    back = read_obj(path)
    assert back["mtllib"] == "mesh.mtl" and back["texture_file"] == "mesh.png"
    assert np.array_equal(back["vertices"].numpy().view(np.uint32), v.view(np.uint32))
    assert back["triangles"].dtype == torch.int32 and np.array_equal(back["triangles"].numpy(), t)
    assert tuple(back["uv"].shape) == (T, 3, 2) and np.array_equal(back["uv"].numpy(), uv.numpy())
    if with_normals:
        assert np.array_equal(back["normals"].numpy().view(np.uint32), n.view(np.uint32))
    else:
        assert back["normals"] is None


def test_obj_of_an_empty_mesh_and_a_missing_mtl(tmp_path, hip_lib_built):
    from pvd.mesh import read_obj, texture_uv, write_obj
    path = str(tmp_path / "e.obj")
    write_obj(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), texture_uv(0, 4), "e.png")
    os.remove(str(tmp_path / "e.mtl"))
    back = read_obj(path)
    assert tuple(back["vertices"].shape) == (0, 3) and tuple(back["triangles"].shape) == (0, 3) and tuple(back["uv"].shape) == (0, 3, 2)
    assert back["texture_file"] is None
    with pytest.raises(ValueError):
        write_obj(path, np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32), np.zeros((2, 3, 2), np.float32), "e.png")
    open(path, "w").write("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError):
        read_obj(path)
