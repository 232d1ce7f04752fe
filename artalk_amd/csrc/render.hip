// FLAME mesh renderer: the first consumer of flame.hip's vertices, a stand-in for the reference's RenderMesh.forward
// (app/flame_model/renderer_utils.py:55-85), which wraps pytorch3d's rasteriser (blur_radius = 0, faces_per_pixel = 1, no back-face
// culling, perspective-correct barycentrics) and its HardPhongShader.  The definition these kernels implement is written out in
// DESIGN.md ("Mesh renderer"); tests/render_ref.py restates it in numpy.  Parity with pytorch3d itself is unpinned.
//   render_project_kernel  per (frame, vertex): view transform, NDC projection, vertex normal gathered over the vertex's faces (CSR,
//                          ascending face order: no floating-point atomics, the sum is reproducible)
//   render_raster_kernel   one wave per (frame, face): walks the face's clamped pixel bounding box in 8x8 tiles, lanes = pixels, and
//                          resolves visibility with a 64-bit unsigned minimum of (bits of depth << 32 | face) per pixel - depth > 0,
//                          so its bits order like its value; the minimum does not depend on the order of arrival and the low word
//                          breaks depth ties towards the lower face index
//   render_shade_kernel    one thread per pixel: reads the winner, recomputes its barycentrics and shades
// Frames are processed in slabs so that the per-pixel key buffer (8 bytes per pixel and frame) stays bounded.
#include "common.h"
#include "device_mem.h"
#include "../../include/artalk_hip.h"

#include <cmath>
#include <string>
#include <vector>

namespace artalk {

struct RenderCam {
    float R[9];      // row-major; p_view = p_world . R + T (row-vector convention)
    float T[3];
    float f;         // focal length in NDC units; principal point 0
    float C[3];      // camera centre, -T . R^T
};

constexpr unsigned long long kRenderEmpty = ~0ull;      // key of a pixel no face covers (the key buffer is filled with 0xFF bytes)

// (no fused multiply-add in the coverage arithmetic: both kernels that evaluate a sample must get the same bits for it)
__device__ __forceinline__ float render_edge(float px, float py, float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}
__device__ __forceinline__ float render_pixel_coord(int i, int S) { return 1.0f - (float)(2 * i + 1) / (float)S; }

// One sample of one face.  a, b, c: (x_ndc, y_ndc, z_view) of its vertices; area: signed area of the edge function, |area| > 1e-8.
// Perspective-correct barycentrics and depth of the pixel centre; false when it is not covered or the sample is skipped.
__device__ __forceinline__ bool render_sample(float px, float py, const float4& a, const float4& b, const float4& c, float area,
                                              float& b0, float& b1, float& b2, float& pz) {
#pragma clang fp contract(off)
    const float w0 = render_edge(px, py, b.x, b.y, c.x, c.y) / area;
    const float w1 = render_edge(px, py, c.x, c.y, a.x, a.y) / area;
    const float w2 = render_edge(px, py, a.x, a.y, b.x, b.y) / area;
    const float t0 = w0 * b.z * c.z, t1 = a.z * w1 * c.z, t2 = a.z * b.z * w2;
    const float den = fmaxf(t0 + t1 + t2, 1e-8f);
    b0 = t0 / den; b1 = t1 / den; b2 = t2 / den;
    pz = b0 * a.z + b1 * b.z + b2 * c.z;
    return w0 > 0.f && w1 > 0.f && w2 > 0.f && !(pz < 0.f);
}

// grid (ceil(V / 256), n frames)
__global__ __launch_bounds__(256) void render_project_kernel(const float* __restrict__ verts /*[n][V][3]*/, const int* __restrict__ faces,
                                                             const int* __restrict__ adj_off /*[V+1]*/, const int* __restrict__ adj /*face ids*/,
                                                             float4* __restrict__ proj /*[n][V]*/, float* __restrict__ nrm /*[n][V][3]*/,
                                                             int V, RenderCam cam) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int t = blockIdx.y;
    const float* vt = verts + (long)t * V * 3;
    const float x = vt[v * 3], y = vt[v * 3 + 1], z = vt[v * 3 + 2];
    const float X = x * cam.R[0] + y * cam.R[3] + z * cam.R[6] + cam.T[0];
    const float Y = x * cam.R[1] + y * cam.R[4] + z * cam.R[7] + cam.T[1];
    const float Z = x * cam.R[2] + y * cam.R[5] + z * cam.R[8] + cam.T[2];
    proj[(long)t * V + v] = make_float4(cam.f * X / Z, cam.f * Y / Z, Z, 0.f);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int i = adj_off[v]; i < adj_off[v + 1]; ++i) {
        const int* fc = faces + (long)adj[i] * 3;
        const float* p0 = vt + (long)fc[0] * 3;
        const float* p1 = vt + (long)fc[1] * 3;
        const float* p2 = vt + (long)fc[2] * 3;
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        nx += ay * bz - az * by;
        ny += az * bx - ax * bz;
        nz += ax * by - ay * bx;
    }
    const float len = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-6f);
    float* o = nrm + ((long)t * V + v) * 3;
    o[0] = nx / len; o[1] = ny / len; o[2] = nz / len;
}

// grid (ceil(F / 4), n frames), 256 threads: wave w of a block rasterises face 4 * blockIdx.x + w
__global__ __launch_bounds__(256) void render_raster_kernel(const float4* __restrict__ proj, const int* __restrict__ faces,
                                                            unsigned long long* __restrict__ keys /*[n][S][S]*/, int V, int F, int S) {
    const int face = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (face >= F) return;
    const int t = blockIdx.y;
    const float4* pt = proj + (long)t * V;
    const float4 a = pt[faces[face * 3]], b = pt[faces[face * 3 + 1]], c = pt[faces[face * 3 + 2]];
    if (!(a.z > 1e-6f && b.z > 1e-6f && c.z > 1e-6f)) return;      // a vertex at or behind the camera plane: the face is not drawn
    const float area = render_edge(c.x, c.y, a.x, a.y, b.x, b.y);
    if (!(fabsf(area) > 1e-8f)) return;
    // pixel centre i sits at 1 - (2 i + 1) / S, so coordinate u falls on index ((1 - u) S - 1) / 2; one index of slack on either side
    // covers the rounding of this estimate (every sample is tested exactly), the clamp keeps every index inside the image
    const float Sf = (float)S;
    const float xmin = fminf(a.x, fminf(b.x, c.x)), xmax = fmaxf(a.x, fmaxf(b.x, c.x));
    const float ymin = fminf(a.y, fminf(b.y, c.y)), ymax = fmaxf(a.y, fmaxf(b.y, c.y));
    const float c_lo = fmaxf(floorf(((1.0f - xmax) * Sf - 1.0f) * 0.5f) - 1.0f, 0.0f);
    const float c_hi = fminf(ceilf(((1.0f - xmin) * Sf - 1.0f) * 0.5f) + 1.0f, Sf - 1.0f);
    const float r_lo = fmaxf(floorf(((1.0f - ymax) * Sf - 1.0f) * 0.5f) - 1.0f, 0.0f);
    const float r_hi = fminf(ceilf(((1.0f - ymin) * Sf - 1.0f) * 0.5f) + 1.0f, Sf - 1.0f);
    if (!(c_lo <= c_hi && r_lo <= r_hi)) return;                   // wholly outside the view
    const int c0 = (int)c_lo, c1 = (int)c_hi, r0 = (int)r_lo, r1 = (int)r_hi;
    unsigned long long* kt = keys + (long)t * S * S;
    const int lr = lane >> 3, lc = lane & 7;
    for (int rb = r0; rb <= r1; rb += 8) {
        const int r = rb + lr;
        const float py = render_pixel_coord(r, S);
        for (int cb = c0; cb <= c1; cb += 8) {
            const int col = cb + lc;
            if (r > r1 || col > c1) continue;
            float b0, b1, b2, pz;
            if (!render_sample(render_pixel_coord(col, S), py, a, b, c, area, b0, b1, b2, pz)) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned int)face;
            unsigned long long* slot = kt + (long)r * S + col;
            // keys only ever decrease, so a key that does not beat a (possibly stale) read cannot beat the current one either
            if (key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, key);
        }
    }
}

__device__ __forceinline__ void render_normalize(float& x, float& y, float& z) {
    const float len = fmaxf(sqrtf(x * x + y * y + z * z), 1e-6f);
    x /= len; y /= len; z /= len;
}

// grid (ceil(S * S / 256), n frames); rgb / alpha / p2f point at the slab's first frame
__global__ __launch_bounds__(256) void render_shade_kernel(const float* __restrict__ verts, const float4* __restrict__ proj,
                                                           const float* __restrict__ nrm, const int* __restrict__ faces,
                                                           const unsigned long long* __restrict__ keys, float* __restrict__ rgb,
                                                           float* __restrict__ alpha, int* __restrict__ p2f, int V, int S, RenderCam cam) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int SS = S * S;
    if (pix >= SS) return;
    const int t = blockIdx.y;
    const unsigned long long key = keys[(long)t * SS + pix];
    float* o = rgb + (long)t * 3 * SS + pix;
    if (key == kRenderEmpty) {
        o[0] = 255.0f; o[SS] = 255.0f; o[2 * (long)SS] = 255.0f;
        alpha[(long)t * SS + pix] = 0.0f;
        if (p2f) p2f[(long)t * SS + pix] = -1;
        return;
    }
    const int face = (int)(unsigned int)(key & 0xFFFFFFFFull);
    const int i0 = faces[face * 3], i1 = faces[face * 3 + 1], i2 = faces[face * 3 + 2];
    const float4 a = proj[(long)t * V + i0], b = proj[(long)t * V + i1], c = proj[(long)t * V + i2];
    const float area = render_edge(c.x, c.y, a.x, a.y, b.x, b.y);
    const int r = pix / S, col = pix - r * S;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, pz;
    (void)render_sample(render_pixel_coord(col, S), render_pixel_coord(r, S), a, b, c, area, b0, b1, b2, pz);
    const float* vt = verts + (long)t * V * 3;
    const float* nt = nrm + (long)t * V * 3;
    float P[3], N[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[k] = b0 * vt[(long)i0 * 3 + k] + b1 * vt[(long)i1 * 3 + k] + b2 * vt[(long)i2 * 3 + k];
        N[k] = b0 * nt[(long)i0 * 3 + k] + b1 * nt[(long)i1 * 3 + k] + b2 * nt[(long)i2 * 3 + k];
    }
    render_normalize(N[0], N[1], N[2]);
    float dx = 0.0f - P[0], dy = 1.0f - P[1], dz = 3.0f - P[2];      // point light at (0, 1, 3)
    render_normalize(dx, dy, dz);
    const float cs = N[0] * dx + N[1] * dy + N[2] * dz;
    float vx = cam.C[0] - P[0], vy = cam.C[1] - P[1], vz = cam.C[2] - P[2];
    render_normalize(vx, vy, vz);
    const float rx = -dx + 2.0f * cs * N[0], ry = -dy + 2.0f * cs * N[1], rz = -dz + 2.0f * cs * N[2];
    const float al = cs > 0.f ? fmaxf(vx * rx + vy * ry + vz * rz, 0.f) : 0.f;
    const float al2 = al * al, al4 = al2 * al2, al8 = al4 * al4;
    const float spec = 0.2f * 0.6f * (al8 * al2);                    // specular 0.6, light's specular 0.2, shininess 10
    const float lit = 0.5f + 0.3f * fmaxf(cs, 0.f);                  // ambient 0.5 + diffuse 0.3
    o[0] = 255.0f * (lit * (142.0f / 255.0f) + spec);
    o[SS] = 255.0f * (lit * (179.0f / 255.0f) + spec);
    o[2 * (long)SS] = 255.0f * (lit * (247.0f / 255.0f) + spec);
    alpha[(long)t * SS + pix] = 1.0f;
    if (p2f) p2f[(long)t * SS + pix] = face;
}

}  // namespace artalk

using namespace artalk;

struct artalk_mesh_renderer {
    int device = 0, V = 0, F = 0, S = 0, slab_max = 0, slab = 0;
    float scale = 1.f;
    DevBuf<int> faces, adj_off, adj;
    DevBuf<float4> proj;                   // the three below: scratch of slab_max frames
    DevBuf<float> nrm;
    DevBuf<unsigned long long> keys;
    std::string err;
};

static thread_local std::string g_render_error;

extern "C" {

const char* artalk_render_last_error(const artalk_mesh_renderer* r) { return r ? r->err.c_str() : g_render_error.c_str(); }

void artalk_render_destroy(artalk_mesh_renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();
    delete r;
}

int artalk_render_create(int device_id, int V, int F, const int32_t* faces_host, int image_size, float scale, artalk_mesh_renderer** out) {
    if (!out) { g_render_error = "out is NULL"; return ARTALK_EINVAL; }
    if (V <= 0) { g_render_error = "V must be positive"; return ARTALK_EINVAL; }
    if (F <= 0) { g_render_error = "F must be positive"; return ARTALK_EINVAL; }
    if (image_size <= 0 || image_size > 16384) { g_render_error = "image_size must be in 1..16384"; return ARTALK_EINVAL; }
    if (!faces_host) { g_render_error = "faces_host is NULL"; return ARTALK_EINVAL; }
    for (int64_t i = 0; i < (int64_t)F * 3; ++i)
        if (faces_host[i] < 0 || faces_host[i] >= V) {
            g_render_error = "face " + std::to_string(i / 3) + " has vertex index " + std::to_string(faces_host[i]) + " outside [0, " +
                             std::to_string(V) + ")";
            return ARTALK_EINVAL;
        }
    // vertex -> faces that hold it, in ascending face order (a face that names a vertex twice is listed once)
    std::vector<int> off(V + 1, 0), adj;
    auto holds_earlier = [&](int f, int k) {
        for (int j = 0; j < k; ++j) if (faces_host[f * 3 + j] == faces_host[f * 3 + k]) return true;
        return false;
    };
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) if (!holds_earlier(f, k)) ++off[faces_host[f * 3 + k] + 1];
    for (int v = 0; v < V; ++v) off[v + 1] += off[v];
    adj.resize(off[V] > 0 ? off[V] : 1);
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int f = 0; f < F; ++f)
            for (int k = 0; k < 3; ++k) if (!holds_earlier(f, k)) adj[fill[faces_host[f * 3 + k]]++] = f;
    }
    if (hipSetDevice(device_id) != hipSuccess) { g_render_error = "hipSetDevice failed"; return ARTALK_EHIP; }
    artalk_mesh_renderer* r = new artalk_mesh_renderer();
    r->device = device_id; r->V = V; r->F = F; r->S = image_size; r->scale = scale;
    const int64_t key_bytes = (int64_t)image_size * image_size * 8;
    int64_t slab = (32ll << 20) / key_bytes;      // 32 MiB of keys: 16 frames at 512 x 512
    r->slab_max = (int)(slab < 1 ? 1 : slab > 64 ? 64 : slab);
    r->slab = r->slab_max;
    if (!r->faces.alloc((size_t)F * 3) || !r->adj_off.alloc((size_t)V + 1) || !r->adj.alloc(adj.size()) ||
        !r->proj.alloc((size_t)r->slab_max * V) || !r->nrm.alloc((size_t)r->slab_max * V * 3) ||
        !r->keys.alloc((size_t)r->slab_max * image_size * image_size)) {
        g_render_error = "hipMalloc failed"; artalk_render_destroy(r); return ARTALK_EHIP;
    }
    (void)hipMemcpy(r->faces.get(), faces_host, (size_t)F * 3 * sizeof(int), hipMemcpyHostToDevice);
    (void)hipMemcpy(r->adj_off.get(), off.data(), (size_t)(V + 1) * sizeof(int), hipMemcpyHostToDevice);
    (void)hipMemcpy(r->adj.get(), adj.data(), adj.size() * sizeof(int), hipMemcpyHostToDevice);
    if (hipDeviceSynchronize() != hipSuccess) { g_render_error = "upload failed"; artalk_render_destroy(r); return ARTALK_EHIP; }
    *out = r;
    return ARTALK_OK;
}

int artalk_render_set_slab(artalk_mesh_renderer* r, int frames) {
    if (!r) { g_render_error = "renderer is NULL"; return ARTALK_EINVAL; }
    if (frames < 0 || frames > r->slab_max) {
        r->err = "slab must be in 0.." + std::to_string(r->slab_max) + " frames (0: the default)";
        return ARTALK_EINVAL;
    }
    r->slab = frames == 0 ? r->slab_max : frames;
    return r->slab;
}

int artalk_render_mesh(artalk_mesh_renderer* r, const float* verts_dev, int T, const float* transform_3x4_host_or_null, float focal_or_0,
                       float* rgb_dev, float* alpha_dev, int32_t* pix_to_face_dev_or_null, void* stream) {
    if (!r) { g_render_error = "renderer is NULL"; return ARTALK_EINVAL; }
    if (!verts_dev || !rgb_dev || !alpha_dev) { r->err = "verts, rgb and alpha must not be NULL"; return ARTALK_EINVAL; }
    if (T < 0) { r->err = "T must not be negative"; return ARTALK_EINVAL; }
    if (T == 0) return ARTALK_OK;
    (void)hipSetDevice(r->device);
    hipStream_t s = (hipStream_t)stream;
    RenderCam cam;
    if (transform_3x4_host_or_null) {
        const float* M = transform_3x4_host_or_null;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) cam.R[i * 3 + j] = M[i * 4 + j];
            cam.T[i] = M[i * 4 + 3];
        }
    } else {      // renderer_utils.py:60-64
        const float Rd[9] = {-1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, -1.f};
        for (int i = 0; i < 9; ++i) cam.R[i] = Rd[i];
        cam.T[0] = 0.f; cam.T[1] = 0.f; cam.T[2] = 2.0f * r->scale;
    }
    cam.f = focal_or_0 != 0.f ? focal_or_0 : 12.0f;
    for (int j = 0; j < 3; ++j) cam.C[j] = -(cam.T[0] * cam.R[j * 3] + cam.T[1] * cam.R[j * 3 + 1] + cam.T[2] * cam.R[j * 3 + 2]);
    const int V = r->V, F = r->F, S = r->S;
    const long SS = (long)S * S;
    int *const faces = r->faces.get(), *const adj_off = r->adj_off.get(), *const adj = r->adj.get();
    float4* const proj = r->proj.get(); float* const nrm = r->nrm.get(); unsigned long long* const keys = r->keys.get();
    for (int t0 = 0; t0 < T; t0 += r->slab) {
        const int n = T - t0 < r->slab ? T - t0 : r->slab;
        const float* verts = verts_dev + (long)t0 * V * 3;
        if (hipMemsetAsync(keys, 0xFF, (size_t)n * SS * 8, s) != hipSuccess) { r->err = "memset failed"; return ARTALK_EHIP; }
        ARTALK_LAUNCH(render_project_kernel, dim3((V + 255) / 256, n), dim3(256), 0, s, verts, faces, adj_off, adj, proj, nrm, V, cam);
        ARTALK_LAUNCH(render_raster_kernel, dim3((F + 3) / 4, n), dim3(256), 0, s, proj, faces, keys, V, F, S);
        ARTALK_LAUNCH(render_shade_kernel, dim3((unsigned)((SS + 255) / 256), n), dim3(256), 0, s, verts, proj, nrm, faces, keys,
                      rgb_dev + (long)t0 * 3 * SS, alpha_dev + (long)t0 * SS,
                      pix_to_face_dev_or_null ? pix_to_face_dev_or_null + (long)t0 * SS : (int32_t*)nullptr, V, S, cam);
    }
    if (hipGetLastError() != hipSuccess) { r->err = "kernel launch failed"; return ARTALK_EHIP; }
    return ARTALK_OK;
}

}  // extern "C"
