// Mesh rendering into every view of a ragged batch (the device side of `eval_single.py --draw`; replaces the host loop of
// lib/utils/testing.py:101-192 upstream: opendr / OpenGL per view behind a device-to-host copy of every mesh).  No MFMA: VALU and LDS
// work, wave64, plain vector stores.  Three kernels:
//   render_vertex_kernel   (mesh, view, vertex): master -> camera frame, pinhole projection, vertex normal from the vertex->face
//                          CSR table (in the table's order: no float atomics, no scatter), Lambert colour under point lights
//   render_raster_kernel   (mesh, view, 16x16 pixel tile): faces binned per 256-face chunk into an LDS list, then every pixel of the
//                          tile walks the list (inside test, perspective-correct barycentrics, depth test)
//   skeleton_kernel        (view, pixel): 21 discs + 20 capsules of the 2-D hand skeleton painted over an image
// Conventions (ours; DESIGN.md section 7 "R"): the sample point of pixel (x, y) is (x, y) in the intrinsics' pixel coordinates; top-left
// fill rule; no back-face culling; no anti-aliasing.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int RT = 16;            // tile side: 16 x 16 pixels = one pixel per thread of a 256-thread block
constexpr int RCHUNK = 256;       // faces binned per pass = list capacity: a chunk's list can never overflow
constexpr int RWORDS = 17;        // words of a binned face: 3 edges x (anchor u, anchor v, s*dv, s*du) | 1/z of the 3 vertices | id, fill bits

// largest b with offs[b] <= v: the sample that owns view v (samples without views are passed over)
__device__ __forceinline__ int sample_of_view(const int* __restrict__ offs, int B, int v) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// master -> camera frame with the inverted extrinsic (the fma chain of project_table_kernel, merge.hip)
__device__ __forceinline__ float3 to_camera(const float* T, const float* __restrict__ p) {
  const float px = p[0], py = p[1], pz = p[2];
  return make_float3(fmaf(T[2], pz, fmaf(T[1], py, T[0] * px)) + T[3], fmaf(T[6], pz, fmaf(T[5], py, T[4] * px)) + T[7],
                     fmaf(T[10], pz, fmaf(T[9], py, T[8] * px)) + T[11]);
}

}  // namespace

// vtx (M, view capacity = gridDim.y, V, 6) = (u, v, z, r, g, b) per vertex; with uv_out (BN, V, 2) the kernel stops behind the projection and writes the
// pixel coordinates only (poem_project_points: faces, CSR, lights and vtx are not read then; M = 1).
__global__ void __launch_bounds__(256) render_vertex_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                            const int* __restrict__ vf_off, const int* __restrict__ vf_faces,
                                                            const float* __restrict__ intr, const float* __restrict__ extr,
                                                            const int* __restrict__ view_offsets, const float* __restrict__ lights,
                                                            int nlights, const float* __restrict__ albedo, float* __restrict__ vtx,
                                                            float* __restrict__ uv_out, int B, int V, int F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int v = blockIdx.y, m = blockIdx.z;
  const int BN = view_offsets[B];
  if (v >= BN) return;                                                  // (block-uniform)
  __shared__ float T[16];                                               // camera -> master inverted by the block itself, as
  if (threadIdx.x == 0) invert4x4(extr + (size_t)v * 16, T);            // input_tables_kernel does (common.h invert4x4)
  __syncthreads();
  if (i >= V) return;
  const int b = sample_of_view(view_offsets, B, v);
  const float* K = intr + (size_t)v * 9;
  const float* mesh = verts + ((size_t)m * B + b) * (size_t)V * 3;
  const float3 p = to_camera(T, mesh + (size_t)i * 3);
  const float u = K[0] * (p.x / p.z) + K[2], w = K[4] * (p.y / p.z) + K[5];
  if (uv_out) {
    reinterpret_cast<float2*>(uv_out)[(size_t)v * V + i] = make_float2(u, w);
    return;
  }
  // vertex normal: the sum of (b - a) x (c - a) over the faces around the vertex, in the CSR table's order
  const int nnz = 3 * F;
  const int beg = min(max(vf_off[i], 0), nnz), end = min(max(vf_off[i + 1], beg), nnz);
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (int k = beg; k < end; ++k) {
    const int f = vf_faces[k];
    if (f < 0 || f >= F) continue;
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) continue;
    const float3 a = to_camera(T, mesh + (size_t)ia * 3), bb = to_camera(T, mesh + (size_t)ib * 3), c = to_camera(T, mesh + (size_t)ic * 3);
    const float e1x = bb.x - a.x, e1y = bb.y - a.y, e1z = bb.z - a.z, e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
    nx += e1y * e2z - e1z * e2y;
    ny += e1z * e2x - e1x * e2z;
    nz += e1x * e2y - e1y * e2x;
  }
  const float n2 = nx * nx + ny * ny + nz * nz;
  const float ninv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;      // a vertex without faces (or with zero-area ones only) is unlit
  nx *= ninv, ny *= ninv, nz *= ninv;
  float sr = 0.f, sg = 0.f, sb = 0.f;
  for (int l = 0; l < nlights; ++l) {
    const float* L = lights + l * 6;
    const float dx = L[0] - p.x, dy = L[1] - p.y, dz = L[2] - p.z;
    const float d2 = dx * dx + dy * dy + dz * dz;
    const float lam = d2 > 0.f ? fmaxf(0.f, (nx * dx + ny * dy + nz * dz) / sqrtf(d2)) : 0.f;
    sr = fmaf(L[3], lam, sr), sg = fmaf(L[4], lam, sg), sb = fmaf(L[5], lam, sb);
  }
  float* o = vtx + (((size_t)m * gridDim.y + v) * (size_t)V + i) * 6;      // the workspace is laid out for the views the launch covers
  reinterpret_cast<float2*>(o)[0] = make_float2(u, w);
  reinterpret_cast<float2*>(o)[1] = make_float2(p.z, fminf(fmaxf(albedo[0] * sr, 0.f), 1.f));
  reinterpret_cast<float2*>(o)[2] = make_float2(fminf(fmaxf(albedo[1] * sg, 0.f), 1.f), fminf(fmaxf(albedo[2] * sb, 0.f), 1.f));
}

// One block per (mesh, view, tile).  Edge functions: the edge between vertices i < j (by vertex index) is evaluated as
//   E(p) = (px - u_i) (v_j - v_i) - (py - v_i) (u_j - u_i)
// relative to ITS lower-index vertex -- a vertex of the face, so the fp32 products stay a few pixels wide -- by both faces that share
// it, which then take E with opposite signs: the same bits, so no pixel between two faces is claimed by neither or (off the edge) by
// both.  A pixel exactly on an edge belongs to the face whose interior lies to its right, or below it for a horizontal edge (top-left rule).
__global__ void __launch_bounds__(256) render_raster_kernel(const float* __restrict__ vtx, const int* __restrict__ faces,
                                                            const int* __restrict__ view_offsets,
                                                            const unsigned char* __restrict__ background, unsigned char* __restrict__ rgb,
                                                            float* __restrict__ depth, int* __restrict__ face_id, int B, int V, int F, int H,
                                                            int W, int tiles_x, float near_z, int packed) {
  __shared__ float rec[RWORDS][RCHUNK];
  __shared__ int wave_count[4];
  __shared__ unsigned int tile_rgb[RT * RT * 3 / 4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int v = blockIdx.y, m = blockIdx.z;
  const int BN = view_offsets[B];
  if (v >= BN) return;                                                  // (block-uniform)
  const int x0 = ((int)blockIdx.x % tiles_x) * RT, y0 = ((int)blockIdx.x / tiles_x) * RT;
  const int px = x0 + (t & 15), py = y0 + (t >> 4);
  const float fx = (float)px, fy = (float)py;
  const float tx0 = (float)x0, ty0 = (float)y0, tx1 = (float)min(x0 + RT - 1, W - 1), ty1 = (float)min(y0 + RT - 1, H - 1);
  const float* mv = vtx + ((size_t)m * gridDim.y + v) * (size_t)V * 6;      // (both launches cover the same view capacity)
  float best = __builtin_inff(), bw0 = 0.f, bw1 = 0.f, bw2 = 0.f;
  int best_id = -1;

  for (int c0 = 0; c0 < F; c0 += RCHUNK) {
    // ---- setup: one face per thread ----
    const int f = c0 + t;
    bool keep = false;
    int id[3];
    float pu[3], pv[3], pz[3], area2 = 0.f;
    if (f < F) {
      id[0] = faces[3 * f], id[1] = faces[3 * f + 1], id[2] = faces[3 * f + 2];
      if ((unsigned)id[0] < (unsigned)V && (unsigned)id[1] < (unsigned)V && (unsigned)id[2] < (unsigned)V) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float2 a = reinterpret_cast<const float2*>(mv + (size_t)id[k] * 6)[0];
          pu[k] = a.x, pv[k] = a.y, pz[k] = mv[(size_t)id[k] * 6 + 2];
        }
        area2 = __fsub_rn(__fmul_rn(pu[1] - pu[0], pv[2] - pv[0]), __fmul_rn(pv[1] - pv[0], pu[2] - pu[0]));
        const float umin = fminf(pu[0], fminf(pu[1], pu[2])), umax = fmaxf(pu[0], fmaxf(pu[1], pu[2]));
        const float vmin = fminf(pv[0], fminf(pv[1], pv[2])), vmax = fmaxf(pv[0], fmaxf(pv[1], pv[2]));
        // (every comparison is false for a NaN: such a face is dropped)
        keep = pz[0] >= near_z && pz[1] >= near_z && pz[2] >= near_z && (area2 > 0.f || area2 < 0.f) && umax >= tx0 && umin <= tx1 &&
               vmax >= ty0 && vmin <= ty1 && fabsf(umin) < 1e9f && fabsf(umax) < 1e9f && fabsf(vmin) < 1e9f && fabsf(vmax) < 1e9f;
      }
    }
    // ---- compaction: ballot + prefix count inside the wave, wave totals through LDS (the faces keep their order) ----
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = wave_count[k];
      base += k < wave ? c : 0;
      total += c;
    }
    if (keep) {
      const int slot = base + before;
      const float orient = area2 > 0.f ? -1.f : 1.f;      // interior side of an edge taken in the face's own direction
      int fill = 0;
#pragma unroll
      for (int e = 0; e < 3; ++e) {                        // edge e lies opposite vertex e: from vertex e+1 to vertex e+2
        const int a = (e + 1) % 3, b2 = (e + 2) % 3;
        const bool fwd = id[a] < id[b2];
        const int i = fwd ? a : b2, j = fwd ? b2 : a;
        const float s = fwd ? orient : -orient;
        const float sdv = s * (pv[j] - pv[i]), sdu = s * (pu[j] - pu[i]);
        rec[4 * e + 0][slot] = pu[i];
        rec[4 * e + 1][slot] = pv[i];
        rec[4 * e + 2][slot] = sdv;
        rec[4 * e + 3][slot] = sdu;
        fill |= (sdv > 0.f || (sdv == 0.f && sdu < 0.f)) ? (1 << e) : 0;
      }
      rec[12][slot] = 1.0f / pz[0];
      rec[13][slot] = 1.0f / pz[1];
      rec[14][slot] = 1.0f / pz[2];
      rec[15][slot] = __int_as_float(f);
      rec[16][slot] = __int_as_float(fill);
    }
    __syncthreads();
    // ---- every pixel of the tile walks the chunk's list ----
    for (int k = 0; k < total; ++k) {
      float E[3];
#pragma unroll
      for (int e = 0; e < 3; ++e)
        E[e] = __fmaf_rn(__fsub_rn(fx, rec[4 * e][k]), rec[4 * e + 2][k], -__fmul_rn(__fsub_rn(fy, rec[4 * e + 1][k]), rec[4 * e + 3][k]));
      const int fill = __float_as_int(rec[16][k]);
      const bool in = (E[0] > 0.f || (E[0] == 0.f && (fill & 1))) && (E[1] > 0.f || (E[1] == 0.f && (fill & 2))) &&
                      (E[2] > 0.f || (E[2] == 0.f && (fill & 4)));
      if (in) {
        const float q0 = E[0] * rec[12][k], q1 = E[1] * rec[13][k], q2 = E[2] * rec[14][k];
        const float S = (E[0] + E[1]) + E[2], Tq = (q0 + q1) + q2;
        const float z = S / Tq;
        if (z < best) {              // lists are walked in face order: at equal depth the lower face index stays
          const float r = 1.0f / Tq;
          best = z, best_id = __float_as_int(rec[15][k]);
          bw0 = q0 * r, bw1 = q1 * r, bw2 = q2 * r;
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue ----
  const bool inside = px < W && py < H;
  const size_t pix = ((size_t)v * H + (inside ? py : 0)) * (size_t)W + (inside ? px : 0);     // within one view plane stack
  const size_t opix = (size_t)m * BN * (size_t)H * W + pix;
  unsigned char c[3] = {255, 255, 255};
  if (best_id >= 0) {
    const int i0 = faces[3 * best_id], i1 = faces[3 * best_id + 1], i2 = faces[3 * best_id + 2];
    const float* a = mv + (size_t)i0 * 6 + 3;
    const float* b2 = mv + (size_t)i1 * 6 + 3;
    const float* c2 = mv + (size_t)i2 * 6 + 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float col = fminf(fmaxf(bw0 * a[k] + bw1 * b2[k] + bw2 * c2[k], 0.f), 1.f);
      c[k] = (unsigned char)min((int)(col * 255.0f), 255);
    }
  } else if (background && inside) {
    c[0] = background[pix * 3], c[1] = background[pix * 3 + 1], c[2] = background[pix * 3 + 2];
  }
  if (inside) {
    if (depth) depth[opix] = best;
    if (face_id) face_id[opix] = best_id;
  }
  if (packed) {
    // a tile row is 48 contiguous bytes: twelve lanes store it as twelve dwords (W % 4 == 0 makes every dword wholly in or out)
    unsigned char* tb = reinterpret_cast<unsigned char*>(tile_rgb);
    tb[t * 3] = c[0], tb[t * 3 + 1] = c[1], tb[t * 3 + 2] = c[2];
    __syncthreads();
    if (t < RT * 12) {
      const int row = t / 12, d = t % 12;
      const int y = y0 + row;
      if (y < H && x0 * 3 + 4 * d + 4 <= W * 3) {
        unsigned char* dst = rgb + ((size_t)m * BN + v) * (size_t)H * W * 3 + ((size_t)y * W + x0) * 3 + 4 * d;
        *reinterpret_cast<unsigned int*>(dst) = tile_rgb[row * 12 + d];
      }
    }
  } else if (inside) {
    rgb[opix * 3] = c[0], rgb[opix * 3 + 1] = c[1], rgb[opix * 3 + 2] = c[2];
  }
}

// image, out (views, H, W, 3); joints (views, 21, 2) pixel coordinates; colours (21, 3) in [0, 1].  Joint j paints its disc (radius 6)
// and the capsule (half-width 1.5) to its parent -- the wrist for j = 4k + 1, j - 1 otherwise (draw_2d_skeleton,
// lib/viztools/draw.py:297-334 upstream) -- over what the joints before it painted.  Hard edges: no anti-aliasing.
// (image and out may be the same buffer: neither is __restrict__; a thread reads and writes its own pixel only)
__global__ void __launch_bounds__(256) skeleton_kernel(const unsigned char* image, const float* __restrict__ joints,
                                                       const float* __restrict__ colours, unsigned char* out, int H, int W) {
  __shared__ float jx[21], jy[21];
  __shared__ unsigned char col[63];
  const int view = blockIdx.y, t = threadIdx.x;
  if (t < 21) {
    jx[t] = joints[((size_t)view * 21 + t) * 2];
    jy[t] = joints[((size_t)view * 21 + t) * 2 + 1];
  } else if (t >= 64 && t < 127) {
    col[t - 64] = (unsigned char)min((int)(fminf(fmaxf(colours[t - 64], 0.f), 1.f) * 255.0f), 255);
  }
  __syncthreads();
  const long idx = (long)blockIdx.x * 256 + t;
  if (idx >= (long)H * W) return;
  const float x = (float)(idx % W), y = (float)(idx / W);
  int hit = -1;
  for (int j = 0; j < 21; ++j) {
    const float dx = x - jx[j], dy = y - jy[j];
    bool on = dx * dx + dy * dy <= 36.0f;
    if (j > 0) {
      const int p = (j & 3) == 1 ? 0 : j - 1;
      const float ax = jx[p], ay = jy[p];
      const float sx = jx[j] - ax, sy = jy[j] - ay, qx = x - ax, qy = y - ay;
      const float len2 = sx * sx + sy * sy;
      const float s = len2 > 0.f ? fminf(fmaxf((qx * sx + qy * sy) / len2, 0.f), 1.f) : 0.f;
      const float ex = qx - s * sx, ey = qy - s * sy;
      on = on || ex * ex + ey * ey <= 2.25f;
    }
    if (on) hit = j;
  }
  const size_t o = ((size_t)view * H * W + (size_t)idx) * 3;
  if (hit >= 0) {
    out[o] = col[3 * hit], out[o + 1] = col[3 * hit + 1], out[o + 2] = col[3 * hit + 2];
  } else {
    out[o] = image[o], out[o + 1] = image[o + 1], out[o + 2] = image[o + 2];
  }
}

extern "C" hipError_t poem_launch_render_vertices(const float* verts, const int* faces, const int* vf_off, const int* vf_faces,
                                                  const float* intr, const float* extr, const int* view_offsets, const float* lights,
                                                  int nlights, const float* albedo, float* vtx, float* uv_out, int M, int B, int V, int F,
                                                  int view_cap, hipStream_t s) {
  hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)view_cap, (unsigned)M), dim3(256), 0, s, verts, faces,
                     vf_off, vf_faces, intr, extr, view_offsets, lights, nlights, albedo, vtx, uv_out, B, V, F);
  return hipGetLastError();
}

extern "C" hipError_t poem_launch_render_raster(const float* vtx, const int* faces, const int* view_offsets, const unsigned char* background,
                                                unsigned char* rgb, float* depth, int* face_id, int M, int B, int V, int F, int H, int W,
                                                float near_z, int view_cap, hipStream_t s) {
  const int tiles_x = (W + RT - 1) / RT, tiles_y = (H + RT - 1) / RT;
  const int packed = (W % 4 == 0) && (((uintptr_t)rgb & 3) == 0);
  hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)view_cap, (unsigned)M), dim3(256), 0, s, vtx, faces,
                     view_offsets, background, rgb, depth, face_id, B, V, F, H, W, tiles_x, near_z, packed);
  return hipGetLastError();
}

extern "C" hipError_t poem_launch_skeleton(const unsigned char* image, const float* joints, const float* colours, unsigned char* out,
                                           int views, int H, int W, hipStream_t s) {
  hipLaunchKernelGGL(skeleton_kernel, dim3((unsigned)(((long)H * W + 255) / 256), (unsigned)views), dim3(256), 0, s, image, joints, colours,
                     out, H, W);
  return hipGetLastError();
}
