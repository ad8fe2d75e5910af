"""CPU-only checks of what the mesh modules share (connecting_the_dots_amd._meshargs) and of the track iterator of
mesh.TsdfMesh: the three wordings of the [rows,3] check, the threshold `_resolve_bvh` is handed, and `tracks()` against
`track(b)` on a hand-built mesh."""
import unittest.mock as mock

import pytest
import torch

from connecting_the_dots_amd.renderer import MeshBVH                 # the class itself: a test below patches the module's


def _fake_bvh(verts, faces, usable=True):
    b = MeshBVH.__new__(MeshBVH)                                     # the build needs a GPU; `matches` and `usable` do not
    b.verts, b.faces, b.usable = verts, faces, usable
    return b


def test_the_three_wordings_of_the_shape_check():
    from connecting_the_dots_amd import _meshargs
    f32, i32 = torch.float32, torch.int32
    with mock.patch.object(_meshargs, "_check", lambda *a, **k: None):    # the device check comes first: step over it
        for bad in (torch.zeros(4), torch.zeros(4, 2), torch.zeros(2, 4, 3)):
            with pytest.raises(RuntimeError) as e:
                _meshargs._nx3(bad, "w", "points", f32)
            assert str(e.value) == "w: points must be shaped [n,3], got %s" % (tuple(bad.shape),)
            with pytest.raises(RuntimeError) as e:
                _meshargs._nx3(bad.int(), "w", "faces", i32, letter="m")
            assert str(e.value) == "w: faces must be shaped [m,3], got %s" % (tuple(bad.shape),)
        with pytest.raises(RuntimeError) as e:
            _meshargs._nx3(torch.zeros(4, 3), "w", "normals", f32, rows=5)
        assert str(e.value) == "w: normals must be shaped [5,3], got (4, 3)"
        with pytest.raises(RuntimeError) as e:
            _meshargs._nx3(torch.zeros(5, 2), "w", "verts", f32, 5)
        assert str(e.value) == "w: verts must be shaped [5,3], got (5, 2)"
        t = torch.zeros(5, 3)
        assert _meshargs._nx3(t, "w", "verts", f32, rows=5) is t and _meshargs._nx3(t, "w", "verts", f32) is t
        assert _meshargs._nx3(torch.zeros(0, 3), "w", "verts", f32, rows=0).shape == (0, 3)
    with pytest.raises(RuntimeError, match="w: verts must be a CUDA tensor"):   # not stepped over: the device comes first
        _meshargs._nx3(torch.zeros(4, 2, dtype=torch.float64), "w", "verts", f32)


def test_resolve_bvh_honours_the_threshold_it_is_given(monkeypatch):
    from connecting_the_dots_amd import _meshargs, renderer
    v, f = torch.zeros(5, 3), torch.zeros(8, 3, dtype=torch.int32)
    built = []
    monkeypatch.setattr(renderer, "MeshBVH", lambda *a: built.append(a) or _fake_bvh(*a))   # 'auto' builds: no GPU here
    assert _meshargs._resolve_bvh("auto", v, f, "w", 9) is None and built == []          # below the threshold: no build
    assert _meshargs._resolve_bvh("auto", v, f, "w", 4096) is None and built == []
    bad = f.clone()
    bad[3, 1] = 5                                                       # a face the tree's build may not read
    assert _meshargs._resolve_bvh("auto", v, bad, "w", 8) is None and built == []
    tree = _meshargs._resolve_bvh("auto", v, f, "w", 8)                 # at the threshold: one build, of these tensors
    assert len(built) == 1 and tree.verts is v and tree.faces is f
    monkeypatch.undo()
    good = _fake_bvh(v, f)
    for min_faces in (0, 8, 10 ** 9):                                   # a given tree does not look at the threshold
        assert _meshargs._resolve_bvh(good, v, f, "w", min_faces) is good
        assert _meshargs._resolve_bvh(None, v, f, "w", min_faces) is None
        assert _meshargs._resolve_bvh(_fake_bvh(v, f, usable=False), v, f, "w", min_faces) is None   # unusable: brute force
        for foreign in (_fake_bvh(v.clone(), f), _fake_bvh(v, f.clone()), _fake_bvh(v[:4], f)):
            with pytest.raises(RuntimeError, match="w: bvh was built from other verts / faces tensors"):
                _meshargs._resolve_bvh(foreign, v, f, "w", min_faces)
        for wrong in ("bvh", 3, (v, f)):
            with pytest.raises(RuntimeError, match="w: bvh must be None, 'auto' or a renderer.MeshBVH"):
                _meshargs._resolve_bvh(wrong, v, f, "w", min_faces)


def test_tracks_yields_what_track_gives():
    from connecting_the_dots_amd import mesh
    verts = torch.arange(21, dtype=torch.float32).reshape(7, 3)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 5, 6]], dtype=torch.int32)
    for normals in (None, -verts):
        m = mesh.TsdfMesh(verts, torch.arange(7), normals, faces, torch.tensor([7, 0]), torch.tensor([3, 0]),
                          [(7, 3), (0, 0)])
        got = list(m.tracks())
        assert m.n_tracks == 2 and [g[0] for g in got] == [0, 1] and [g[4] for g in got] == [0, 7]
        for b, v, f, n, v0 in got:
            want = m.track(b)
            assert torch.equal(v, want[0]) and torch.equal(f, want[1]) and v.data_ptr() == want[0].data_ptr()
            assert (n is None and want[2] is None) if normals is None else torch.equal(n, want[2])
            assert torch.equal(m.verts[v0:v0 + v.shape[0]], v)
        assert got[0][1].shape == (7, 3) and got[0][2].shape == (3, 3)
        assert got[1][1].shape == (0, 3) and got[1][2].shape == (0, 3)       # the empty second track
    three = mesh.TsdfMesh(verts, torch.arange(7), None, faces, None, None, [(2, 1), (0, 0), (5, 2)])
    assert [(g[0], g[4], g[1].shape[0], g[2].shape[0]) for g in three.tracks()] == [(0, 0, 2, 1), (1, 2, 0, 0), (2, 2, 5, 2)]
    assert torch.equal(list(three.tracks())[2][2], faces[1:])
    assert list(mesh.TsdfMesh(verts[:0], torch.arange(0), None, faces[:0], None, None, []).tracks()) == []
