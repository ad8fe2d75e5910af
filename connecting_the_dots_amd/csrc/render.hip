// render.hip -- synthetic structured-light rendering: the reference's brute-force ray caster
// with projector inpainting, RenderProjectorFunctor<float>::operator()
// (renderer/render/render.h:251-364; ray/mesh intersection geometry.h:201-258, camera
// render.h:12-87, Phong shader geometry.h:262-292, bilinear pattern fetch render.h:228-249; launched by
// render_gpu.cu through iterate_cuda, one thread per camera pixel).
//
// The camera, ray_tri and the shading after the hit live in ctd_render.h (shared with the BVH caster).
// One thread per camera pixel; the mesh streams through LDS in tiles of gathered vertex triples that every lane
// reads at the same address (broadcast), once for the camera ray and once for the shadow ray from the
// projector.  Every expression keeps the reference's operation order and the library is built without FMA
// contraction, so depth, hit face and the projected pattern are bit-identical to the reference CPU build; the
// shaded ambient image is too whenever the specular weight ks is 0 (the data generator's setting,
// data/create_syn_data.py:155), otherwise it differs by powf's last bits.
#include "ctd_common.h"
#include "ctd_render.h"

namespace ctd {

constexpr int kFaceTile = 256;     // faces per LDS tile: 256 x 3 vertices x float4 = 12 KB

// nearest hit of one ray per thread against the whole mesh (geometry.h:235-258); all threads of the workgroup
// take part in the staging even if their ray is not live
__device__ inline bool ray_mesh(float (*tile)[4], const float* orig, const float* dir, bool live,
                                const float* __restrict__ verts, const int* __restrict__ faces, int n_faces,
                                int& face_idx, float& t, float& u, float& v) {
  t = FLT_MAX;
  bool valid = false;
  for (int base = 0; base < n_faces; base += kFaceTile) {
    const int n = min(kFaceTile, n_faces - base);
    __syncthreads();
    for (int i = threadIdx.x; i < n * 3; i += blockDim.x) {
      const int vi = faces[(long)base * 3 + i];
      tile[i][0] = verts[(long)vi * 3 + 0];
      tile[i][1] = verts[(long)vi * 3 + 1];
      tile[i][2] = verts[(long)vi * 3 + 2];
    }
    __syncthreads();
    if (!live) continue;
    for (int f = 0; f < n; ++f) {
      float ft, fu, fv;
      if (ray_tri(orig, dir, tile[3 * f], tile[3 * f + 1], tile[3 * f + 2], ft, fu, fv) && ft < t) {
        face_idx = base + f;
        t = ft;
        u = fu;
        v = fv;
        valid = true;
      }
    }
  }
  return valid;
}

__global__ __launch_bounds__(256) void render_proj_kernel(const float* __restrict__ verts, const float* __restrict__ colors,
                                                          const int* __restrict__ faces, int n_faces, CamDev cam,
                                                          CamDev proj, float ka, float kd, float ks, float alpha,
                                                          const float* __restrict__ pattern, float d_alpha, float d_beta,
                                                          float* __restrict__ depth, float* __restrict__ color,
                                                          float* __restrict__ normal) {
  __shared__ float tile[kFaceTile * 3][4];
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_img = idx < cam.width * cam.height;
  const int h = idx / cam.width, w = idx % cam.width;
  const float orig[3] = {cam.C[0], cam.C[1], cam.C[2]};
  float dir[3];
  camera_ray(cam, h, w, dir);
  int face_idx = 0;
  float t, tu, tv;
  bool valid = ray_mesh(tile, orig, dir, in_img, verts, faces, n_faces, face_idx, t, tu, tv);
  valid = valid && in_img;
  if (in_img) {
    if (depth) depth[idx] = valid ? t : -1;
    color[idx * 3 + 0] = 0;
    color[idx * 3 + 1] = 0;
    color[idx * 3 + 2] = 0;
  }
  float pt[3] = {0.f, 0.f, 0.f}, pdir[3] = {0.f, 0.f, 1.f};
  const float porig[3] = {proj.C[0], proj.C[1], proj.C[2]};
  if (valid) {
    proj_camera_hit(verts, colors, faces, face_idx, orig, dir, t, tu, tv, ka, kd, ks, alpha, normal, idx, porig, pt,
                    pdir);
  }
  // shadow ray: does the projector see the same surface point?
  int p_face = 0;
  float p_t, p_tu, p_tv;
  const bool p_valid = ray_mesh(tile, porig, pdir, valid, verts, faces, n_faces, p_face, p_t, p_tu, p_tv);
  if (!valid || !p_valid) return;
  proj_pattern_fetch(proj, pattern, d_alpha, d_beta, pt, porig, pdir, p_t, color, idx);
}

static int render_mesh_proj_f32(const float* verts, const float* colors, const int* faces, int n_faces,
                                const float* cam_p, int cam_w, int cam_h, const float* proj_p, int proj_w, int proj_h,
                                const float* shader, const float* pattern, float d_alpha, float d_beta, float* depth,
                                float* color, float* normal, hipStream_t stream) {
  const CamDev cam = make_cam(cam_p, cam_w, cam_h), proj = make_cam(proj_p, proj_w, proj_h);
  const long n = (long)cam_w * cam_h;
  hipLaunchKernelGGL(render_proj_kernel, dim3((unsigned)ceil_div(n, 256L)), dim3(256), 0, stream, verts, colors, faces,
                     n_faces, cam, proj, shader[0], shader[1], shader[2], shader[3], pattern, d_alpha, d_beta, depth, color,
                     normal);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

// RenderMeshFunctor<float>::operator() (render.h:150-223): camera rays only; the normal buffer receives the
// interpolated vertex normals (flipped towards the camera, not normalised), the colour buffer the Phong-shaded
// interpolated vertex colours.  Buffers may be null like the reference's.
__global__ __launch_bounds__(256) void render_mesh_kernel(const float* __restrict__ verts, const float* __restrict__ colors,
                                                          const float* __restrict__ normals, const int* __restrict__ faces,
                                                          int n_faces, CamDev cam, float ka, float kd, float ks, float alpha,
                                                          float* __restrict__ depth, float* __restrict__ color,
                                                          float* __restrict__ normal) {
  __shared__ float tile[kFaceTile * 3][4];
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in_img = idx < cam.width * cam.height;
  const int h = idx / cam.width, w = idx % cam.width;
  const float orig[3] = {cam.C[0], cam.C[1], cam.C[2]};
  float dir[3];
  camera_ray(cam, h, w, dir);
  int face_idx = 0;
  float t, tu, tv;
  const bool valid = ray_mesh(tile, orig, dir, in_img, verts, faces, n_faces, face_idx, t, tu, tv);
  if (!in_img) return;
  mesh_shade(verts, colors, normals, faces, valid, face_idx, orig, dir, t, tu, tv, ka, kd, ks, alpha, depth, color, normal,
             idx);
}

static int render_mesh_f32(const float* verts, const float* colors, const float* normals, const int* faces, int n_faces,
                           const float* cam_p, int cam_w, int cam_h, const float* shader, float* depth, float* color,
                           float* normal, hipStream_t stream) {
  const CamDev cam = make_cam(cam_p, cam_w, cam_h);
  const long n = (long)cam_w * cam_h;
  hipLaunchKernelGGL(render_mesh_kernel, dim3((unsigned)ceil_div(n, 256L)), dim3(256), 0, stream, verts, colors, normals,
                     faces, n_faces, cam, shader[0], shader[1], shader[2], shader[3], depth, color, normal);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_render_mesh_proj_f32(const float* verts, const float* colors, int n_verts, const int* faces, int n_faces,
                             const float* cam, int cam_width, int cam_height, const float* proj, int proj_width,
                             int proj_height, const float* shader, const float* pattern, float d_alpha, float d_beta,
                             float* depth, float* color, float* normal, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || cam_width <= 0 || cam_height <= 0 || proj_width <= 0 || proj_height <= 0 ||
      (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!cam || !proj || !shader || !pattern || !color || (n_faces > 0 && (!verts || !colors || !faces)))
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_proj_f32(verts, colors, faces, n_faces, cam, cam_width, cam_height, proj, proj_width, proj_height,
                              shader, pattern, d_alpha, d_beta, depth, color, normal, (hipStream_t)stream);
}

int ctd_render_mesh_f32(const float* verts, const float* colors, const float* normals, int n_verts, const int* faces,
                        int n_faces, const float* cam, int cam_width, int cam_height, const float* shader, float* depth,
                        float* color, float* normal, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || cam_width <= 0 || cam_height <= 0 || (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!cam || !shader || (n_faces > 0 && (!verts || !faces))) return CTD_ERR_INVALID_ARG;
  if (n_faces > 0 && ((color && !colors) || ((color || normal) && !normals))) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_f32(verts, colors, normals, faces, n_faces, cam, cam_width, cam_height, shader, depth, color, normal,
                         (hipStream_t)stream);
}

}  // extern "C"
