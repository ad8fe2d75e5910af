"""MI355X-native disparity hot path of autonomousvision/connecting_the_dots.

`connecting_the_dots_amd.torchext` mirrors the reference's `torchext.functions` /
`torchext.modules` API (torchext/functions.py, torchext/modules.py); the arithmetic runs in
hand-written HIP kernels (csrc/) behind the C ABI of include/ctd_hip.h.

    torchext.functions   the import surface: every op by name, nothing else (`__all__`)
    torchext.modules     the nn.Module wrappers (CoordConv2d, LCN, the loss modules)
    torchext.<family>    the wrappers themselves, one module per kernel family: nn_ops, ncc, lcn_ops, photometric,
                         costvol_ops, subpixel, validity, band, sgm, disp_filter, multiview, tsdf, losses; what they
                         share is in torchext._common (checks, launch plumbing) and torchext._track (posed views)
    _lib                 ctypes binding of libctd_hip.so; build: `python -m connecting_the_dots_amd.build`
    synth, renderer, hyperdepth, nets, train, sharding   the data, model and training side above torchext
    bandsgm              band-limited semi-global matching (include/ext/ctd_hip_band_sgm.h): the band matchers' scores as a
                         band volume of `slots` planes, and SGM aggregation within every pixel's own disparity range
    mesh                 the triangle mesh of a TSDF volume (include/ctd_hip_mesh.h) for renderer.MeshBVH, and PLY files
    meshops              mesh clean-up (include/ctd_hip_mesh_clean.h): connected components, removal of small components,
                         of faces with coincident vertices and of unreferenced vertices, compaction
    mesheval             nearest-face queries (include/ctd_hip_mesh_dist.h) by brute force or through renderer.MeshBVH, surface
                         samples, and the accuracy / completeness / Chamfer / F-score of one mesh against another
    meshcolor            colours for mesh points from a track's views (include/ctd_hip_mesh_color.h): projection, occlusion
                         against the mesh by brute force or through renderer.MeshBVH, bilinear sample, blend of the views
    meshsmooth           the mesh's connectivity by vertex (include/ctd_hip_mesh_smooth.h): one-rings, incident faces, boundary
                         and non-manifold edges; Taubin smoothing over the one-rings; area-weighted vertex normals
    meshsimplify         mesh simplification (include/ctd_hip_mesh_simplify.h): vertex clustering on a uniform grid, every
                         cluster's vertex at the minimum of its summed plane quadrics, duplicate faces dropped
    meshsdf              signed nearest-face queries (include/ctd_hip_mesh_sdf.h): the side by the angle-weighted pseudonormal,
                         a distance cutoff, a mesh back into a TSDF volume, the signed error of one mesh against another
    meshreg              point-to-mesh ICP (include/ext/ctd_hip_mesh_register.h): the 6 x 6 system of a point set under K poses
                         against a mesh, the pose update, the loop with the last round's faces as a hint, a mesh registered
                         to a mesh through its surface samples, and the reconstruction error after alignment
    meshrobust           robust point-to-mesh ICP (include/ext/ctd_hip_mesh_robust.h): meshreg's system with Huber or Tukey
                         weights, matches on the rim of an open mesh rejected and a normal gate; the per-face rim table,
                         the scale from a round's residuals, the loop, and the reconstruction error after alignment
    meshglobal           global point-to-mesh registration (include/ext/ctd_hip_mesh_global.h): a grid of rotations x offsets
                         scored exactly against a volume of uint8 distance levels, the best few refined by meshreg's or
                         meshrobust's loop and ranked by the point metric; registration from any starting orientation
    pointcloud           bare point sets (include/ext/ctd_hip_point_cloud.h): exact k-nearest-neighbours over a sorted grid of
                         cells (PointGrid, knn), the statistical outlier mask, covariance normals and the voxel-mean
                         down-sample that rest on it; for fused points before they meet a mesh
    _meshargs            what the seven mesh modules and renderer share above the C calls: argument checks, the choice of
                         a tree for a query, the steps of the *_tsdf_mesh functions
"""
from . import torchext  # noqa: F401

__version__ = "0.1.0"
