"""CPU-only checks of the volume-free cost argmin (ctd_costvol_argmin_f32): the workspace query, argument validation
before any HIP call and the Python surface."""


def test_workspace_query():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    for ty in range(4):
        for per_frame in (0, 1):
            n = L.ctd_costvol_argmin_workspace_bytes(1, 1024, 1024, 256, 9, ty, per_frame)
            assert n > 0
            # O(frames * H * W * ceil(D / 128)): far below one f32 volume (1 GiB here)
            assert n < 0.05 * 1024 * 1024 * 256 * 4
    assert L.ctd_costvol_argmin_workspace_bytes(2, 1024, 1024, 256, 9, 3, 0) > \
        L.ctd_costvol_argmin_workspace_bytes(1, 1024, 1024, 256, 9, 3, 0)
    assert L.ctd_costvol_argmin_workspace_bytes(1, 1024, 1024, 257, 9, 3, 0) > \
        L.ctd_costvol_argmin_workspace_bytes(1, 1024, 1024, 256, 9, 3, 0)
    # empty / invalid requests need none
    assert L.ctd_costvol_argmin_workspace_bytes(0, 1024, 1024, 256, 9, 3, 0) == 0
    assert L.ctd_costvol_argmin_workspace_bytes(1, 0, 1024, 256, 9, 3, 0) == 0
    assert L.ctd_costvol_argmin_workspace_bytes(1, 1024, 1024, 0, 9, 3, 0) == 0
    assert L.ctd_costvol_argmin_workspace_bytes(1, 64, 64, 16, 8, 3, 0) == 0
    assert L.ctd_costvol_argmin_workspace_bytes(1, 64, 64, 16, 9, 7, 0) == 0


def test_validation_needs_no_gpu():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    args = lambda bs, ty, rel=1e-5, stride=0: (None, None, stride, None, None, 1, 8, 8, 4, bs, ty, 0.5, rel, None, 0, -1,
                                               None)
    assert L.ctd_costvol_argmin_f32(*args(8, 3)) == 1            # even block size
    assert L.ctd_costvol_argmin_f32(*args(9, 7)) == 1            # bad type
    assert L.ctd_costvol_argmin_f32(*args(9, -1)) == 1
    assert L.ctd_costvol_argmin_f32(*args(9, 3, float("nan"))) == 1
    assert L.ctd_costvol_argmin_f32(*args(9, 3, 1e-5, 7)) == 1   # pattern stride neither 0 nor H * W
    # no frames: nothing to do, nothing touched
    assert L.ctd_costvol_argmin_f32(None, None, 0, None, None, 0, 8, 8, 4, 9, 3, 0.5, 1e-5, None, 0, -1, None) == 0


def test_python_surface():
    from connecting_the_dots_amd import torchext as te
    import inspect
    assert callable(te.costvol_argmin)
    sig = inspect.signature(te.costvol_argmin)
    assert list(sig.parameters)[:7] == ["im", "pattern", "n_disps", "block_size", "type", "eps", "rerank_rel"]
    assert sig.parameters["type"].default == "census_sad"
    assert sig.parameters["rerank_rel"].default == 1e-5
