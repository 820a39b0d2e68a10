// oracle/ref/ref_cl_shim.cpp -- TEST INFRASTRUCTURE ONLY.  Links with the REFERENCE's own OpenCL C kernels, compiled for
// the host by clang -x cl (oracle/ref/Makefile), into oracle/_ref/libref_cl_<tf>.so.  Two things live here, both ours:
//   (a) the OpenCL built-ins that translation unit leaves undefined, under their mangled names, each defined exactly as
//       DESIGN.md section 2 ("Semantics fixed where OpenCL leaves them implementation-defined") and oracle/orc_render.c state it;
//   (b) a plain C driver: images and the cache from host arrays, a kernel run over a launch rectangle serially (rows outer,
//       x inner -- the order of orc_render with threads = 1), the atomics logged so that the hit entry and the contribution
//       of every pixel can be handed back.
// Compile with the same clang and -ffp-contract=off as the kernels: the vector types below are clang's ext_vector_type,
// which is what OpenCL C's float3 / float4 / int4 are, so both objects pass them the same way.  refcl_abi_status() proves it.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

typedef float float2 __attribute__((ext_vector_type(2)));
typedef float float3 __attribute__((ext_vector_type(3)));
typedef float float4 __attribute__((ext_vector_type(4)));
typedef int int2 __attribute__((ext_vector_type(2)));
typedef int int4 __attribute__((ext_vector_type(4)));
typedef unsigned uint4 __attribute__((ext_vector_type(4)));

namespace {

enum { ELEM_I8 = 0, ELEM_I16 = 1, ELEM_RGBA8 = 2 };
struct image {
  int32_t w, h, d, elem;
  void *data;
};
typedef image *image_t;   // image2d_t / image3d_t are opaque pointers on this target
typedef void *sampler_t;  // so is sampler_t; the value is the initializer's bits

struct atomic_record {
  int64_t gid;    // y * launch_w + x of the work-item (x + w * (y + h * z) for 3-D launches)
  int64_t word;   // index of the 32-bit word from the registered buffer's base
  int32_t addend; // negative for atomic_sub
};

size_t g_id[3];
int64_t g_gid;
const int32_t *g_atomic_base;
int64_t g_atomic_words;
std::vector<atomic_record> g_log;
bool g_logging;
int64_t g_out_of_range;  // accesses the shim refused because they lie outside the registered buffer / image

// Which bounce depth a path left the volume at (ray_marching.cl:52-62), read off the built-in calls of one work-item after
// its token request: a secondary ray starts with normalize, normalize, fabs (:48-50; the first one after the normal's
// normalize of :42), a bounce at a Hit is normalize, normalize, normalize, fabs (:64-67), an Exit_volume is the read of the
// environment map (:57).  g_exit_depth[k] counts the paths that left after k Hits, that is with i = 8 + k.
struct path_trace { bool active, first; int normalizes, hits; } g_path;
int64_t g_exit_depth[3];
int64_t g_trace_unexpected;
inline void trace_fabs() {
  if (!g_path.active) return;
  const int n = g_path.normalizes - (g_path.first ? 1 : 0);
  if (n == 2) g_path.hits = 0;
  else if (n == 3 && !g_path.first) ++g_path.hits;
  else ++g_trace_unexpected;
  g_path.first = false;
  g_path.normalizes = 0;
}
inline void trace_env_read() {
  if (!g_path.active) return;
  if (g_path.hits < 3 && g_path.normalizes == 0) ++g_exit_depth[g_path.hits];
  else ++g_trace_unexpected;
}

inline int32_t texel(const image *im, int64_t x, int64_t y, int64_t z) {
  const int64_t i = (z * im->h + y) * im->w + x;
  return im->elem == ELEM_I8 ? (int32_t) static_cast<const int8_t *>(im->data)[i] : (int32_t) static_cast<const int16_t *>(im->data)[i];
}
inline bool atomic_in_range(const volatile int32_t *p) {
  const int64_t w = (const int32_t *)p - g_atomic_base;
  if (g_atomic_base && w >= 0 && w < g_atomic_words) return true;
  ++g_out_of_range;
  return false;
}
inline void log_atomic(const volatile int32_t *p, int32_t addend) {
  if (g_logging) g_log.push_back({g_gid, (int64_t)((const int32_t *)p - g_atomic_base), addend});
}

}  // namespace

// ---- (a) the built-ins ------------------------------------------------------------------------------------------------------
extern "C" {

// "integer images with CLK_FILTER_LINEAR are not filtered: texel = floor(coord); CLK_ADDRESS_CLAMP out-of-range or
// NaN -> border 0" (orc_render.c vol_read_f).  A CL_R image returns (r, 0, 0, 1).
int4 cl_read_imagei_3d_f(image_t im, sampler_t, float4 c) __asm__("_Z11read_imagei14ocl_image3d_ro11ocl_samplerDv4_f");
int4 cl_read_imagei_3d_f(image_t im, sampler_t, float4 c) {
  const float gx = floorf(c.x), gy = floorf(c.y), gz = floorf(c.z);
  int4 r = {0, 0, 0, 1};
  if (!(gx >= 0.0f && gy >= 0.0f && gz >= 0.0f && gx < (float)im->w && gy < (float)im->h && gz < (float)im->d)) return r;
  r.x = texel(im, (int64_t)gx, (int64_t)gy, (int64_t)gz);
  return r;
}
// the same with integer coordinates (orc_render.c sdf_read_i)
int4 cl_read_imagei_3d_i(image_t im, sampler_t, int4 c) __asm__("_Z11read_imagei14ocl_image3d_ro11ocl_samplerDv4_i");
int4 cl_read_imagei_3d_i(image_t im, sampler_t, int4 c) {
  int4 r = {0, 0, 0, 1};
  if (c.x < 0 || c.y < 0 || c.z < 0 || c.x >= im->w || c.y >= im->h || c.z >= im->d) return r;
  r.x = texel(im, c.x, c.y, c.z);
  return r;
}
// sampler-less read (reference_volume_clip.cl:13): integer coordinates, border 0
int4 cl_read_imagei_3d_nosmp(image_t im, int4 c) __asm__("_Z11read_imagei14ocl_image3d_roDv4_i");
int4 cl_read_imagei_3d_nosmp(image_t im, int4 c) { return cl_read_imagei_3d_i(im, nullptr, c); }

// "env map: floor(u*w), clamp to edge" (orc_render.c env_texel: float -> int saturating, NaN -> 0)
uint4 cl_read_imageui_2d(image_t im, sampler_t, float2 uv) __asm__("_Z12read_imageui14ocl_image2d_ro11ocl_samplerDv2_f");
uint4 cl_read_imageui_2d(image_t im, sampler_t, float2 uv) {
  auto f2i = [](float v) -> int32_t {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return (int32_t)v;
  };
  int32_t i = f2i(floorf(uv.x * (float)im->w)), j = f2i(floorf(uv.y * (float)im->h));
  if (i < 0) i = 0;
  if (i > im->w - 1) i = im->w - 1;
  if (j < 0) j = 0;
  if (j > im->h - 1) j = im->h - 1;
  trace_env_read();
  const uint8_t *t = static_cast<const uint8_t *>(im->data) + ((int64_t)j * im->w + i) * 4;
  uint4 r = {t[0], t[1], t[2], t[3]};
  return r;
}
// write_imageui on CL_UNSIGNED_INT8 saturates (orc_render.c frame_write); a write outside the image is dropped
void cl_write_imageui_2d(image_t im, int2 p, uint4 c) __asm__("_Z13write_imageui14ocl_image2d_woDv2_iDv4_j");
void cl_write_imageui_2d(image_t im, int2 p, uint4 c) {
  if (p.x < 0 || p.y < 0 || p.x >= im->w || p.y >= im->h) { ++g_out_of_range; return; }
  uint8_t *t = static_cast<uint8_t *>(im->data) + ((int64_t)p.y * im->w + p.x) * 4;
  for (int k = 0; k < 4; ++k) t[k] = c[k] > 255u ? 255 : (uint8_t)c[k];
}
// write_imagei on CL_SIGNED_INT16 saturates; .x is the channel of a CL_R image
void cl_write_imagei_3d(image_t im, int4 p, int4 c) __asm__("_Z12write_imagei14ocl_image3d_woDv4_iS0_");
void cl_write_imagei_3d(image_t im, int4 p, int4 c) {
  if (p.x < 0 || p.y < 0 || p.z < 0 || p.x >= im->w || p.y >= im->h || p.z >= im->d) { ++g_out_of_range; return; }
  const int32_t v = c.x > 32767 ? 32767 : (c.x < -32768 ? -32768 : c.x);
  static_cast<int16_t *>(im->data)[((int64_t)p.z * im->h + p.y) * im->w + p.x] = (int16_t)v;
}

// tf_flush_color_frame's write (histogram.cl:75), which no driver entry runs: defined so that the library links
void cl_write_imagei_2d(image_t im, int2 p, int4 c) __asm__("_Z12write_imagei14ocl_image2d_woDv2_iDv4_i");
void cl_write_imagei_2d(image_t im, int2 p, int4 c) {
  if (p.x < 0 || p.y < 0 || p.x >= im->w || p.y >= im->h) { ++g_out_of_range; return; }
  uint8_t *t = static_cast<uint8_t *>(im->data) + ((int64_t)p.y * im->w + p.x) * 4;
  for (int k = 0; k < 4; ++k) t[k] = c[k] > 255 ? 255 : (c[k] < 0 ? 0 : (uint8_t)c[k]);
}

int cl_width_3d(image_t im) __asm__("_Z15get_image_width14ocl_image3d_ro");
int cl_width_3d(image_t im) { return im->w; }
int cl_height_3d(image_t im) __asm__("_Z16get_image_height14ocl_image3d_ro");
int cl_height_3d(image_t im) { return im->h; }
int cl_depth_3d(image_t im) __asm__("_Z15get_image_depth14ocl_image3d_ro");
int cl_depth_3d(image_t im) { return im->d; }
int cl_width_2d_wo(image_t im) __asm__("_Z15get_image_width14ocl_image2d_wo");
int cl_width_2d_wo(image_t im) { return im->w; }
int cl_height_2d_wo(image_t im) __asm__("_Z16get_image_height14ocl_image2d_wo");
int cl_height_2d_wo(image_t im) { return im->h; }
int cl_width_2d_ro(image_t im) __asm__("_Z15get_image_width14ocl_image2d_ro");
int cl_width_2d_ro(image_t im) { return im->w; }
int cl_height_2d_ro(image_t im) __asm__("_Z16get_image_height14ocl_image2d_ro");
int cl_height_2d_ro(image_t im) { return im->h; }
int4 cl_dim_3d(image_t im) __asm__("_Z13get_image_dim14ocl_image3d_ro");
int4 cl_dim_3d(image_t im) { int4 r = {im->w, im->h, im->d, 0}; return r; }
int2 cl_dim_2d_wo(image_t im) __asm__("_Z13get_image_dim14ocl_image2d_wo");
int2 cl_dim_2d_wo(image_t im) { int2 r = {im->w, im->h}; return r; }

size_t cl_get_global_id(unsigned d) __asm__("_Z13get_global_idj");
size_t cl_get_global_id(unsigned d) { return d < 3 ? g_id[d] : 0; }
sampler_t __translate_sampler_initializer(int v) { return (sampler_t)(intptr_t)v; }

// 32-bit atomics on __global int / uint: the driver runs one work-item at a time, so plain read-modify-write; logged
int32_t cl_atomic_add(volatile int32_t *p, int32_t v) __asm__("_Z10atomic_addPU8CLglobalVii");
int32_t cl_atomic_add(volatile int32_t *p, int32_t v) {
  if (!atomic_in_range(p)) return 0;
  log_atomic(p, v);
  if (g_logging && v == 0x00010000) g_path = {true, true, 0, 0};  // the token request of utility.cl:27
  const int32_t old = *p;
  *p = (int32_t)((uint32_t)old + (uint32_t)v);
  return old;
}
int32_t cl_atomic_sub(volatile int32_t *p, int32_t v) __asm__("_Z10atomic_subPU8CLglobalVii");
int32_t cl_atomic_sub(volatile int32_t *p, int32_t v) {
  if (!atomic_in_range(p)) return 0;
  log_atomic(p, (int32_t)(0u - (uint32_t)v));
  const int32_t old = *p;
  *p = (int32_t)((uint32_t)old - (uint32_t)v);
  return old;
}
int32_t cl_atomic_min(volatile int32_t *p, int32_t v) __asm__("_Z10atomic_minPU8CLglobalVii");
int32_t cl_atomic_min(volatile int32_t *p, int32_t v) {
  if (!atomic_in_range(p)) return 0;
  const int32_t old = *p;
  if (v < old) *p = v;
  return old;
}
int32_t cl_atomic_max(volatile int32_t *p, int32_t v) __asm__("_Z10atomic_maxPU8CLglobalVii");
int32_t cl_atomic_max(volatile int32_t *p, int32_t v) {
  if (!atomic_in_range(p)) return 0;
  const int32_t old = *p;
  if (v > old) *p = v;
  return old;
}
uint32_t cl_atomic_inc(volatile uint32_t *p) __asm__("_Z10atomic_incPU8CLglobalVj");
uint32_t cl_atomic_inc(volatile uint32_t *p) {
  if (!atomic_in_range((volatile int32_t *)p)) return 0;  // histogram.cl:31 indexes past the frame for the top row / column
  const uint32_t old = *p;
  *p = old + 1u;
  return old;
}

// "every float operation is one IEEE-754 binary32 operation in source order"; dot = (x*x' + y*y') + z*z'
// (orc_render.c v_dot), cross as orc_render.c v_cross
float cl_dot3(float3 a, float3 b) __asm__("_Z3dotDv3_fS_");
float cl_dot3(float3 a, float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
float3 cl_cross3(float3 a, float3 b) __asm__("_Z5crossDv3_fS_");
float3 cl_cross3(float3 a, float3 b) {
  float3 r = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
  return r;
}
// "normalize(v) = v / sqrtf((x^2+y^2)+z^2) (three divisions)"; length is that square root
float cl_length3(float3 a) __asm__("_Z6lengthDv3_f");
float cl_length3(float3 a) { return sqrtf(cl_dot3(a, a)); }
float3 cl_normalize3(float3 a) __asm__("_Z9normalizeDv3_f");
float3 cl_normalize3(float3 a) {
  if (g_path.active) ++g_path.normalizes;
  const float l = cl_length3(a);
  float3 r = {a.x / l, a.y / l, a.z / l};
  return r;
}
// "min(a,b) = b<a ? b : a, max(a,b) = a<b ? b : a"
float cl_min(float a, float b) __asm__("_Z3minff");
float cl_min(float a, float b) { return (b < a) ? b : a; }
float cl_max(float a, float b) __asm__("_Z3maxff");
float cl_max(float a, float b) { return (a < b) ? b : a; }
float cl_fabs(float a) __asm__("_Z4fabsf");
float cl_fabs(float a) { trace_fabs(); return fabsf(a); }
// "atan2, asin, pow [and exp, orc_filter.c] return the correctly rounded binary32 value (evaluated in binary64, rounded once)"
float cl_pow(float a, float b) __asm__("_Z3powff");
float cl_pow(float a, float b) { return (float)pow((double)a, (double)b); }
float cl_atan2(float y, float x) __asm__("_Z5atan2ff");
float cl_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }
float cl_asin(float a) __asm__("_Z4asinf");
float cl_asin(float a) { return (float)asin((double)a); }
float cl_exp(float a) __asm__("_Z3expf");
float cl_exp(float a) { return (float)exp((double)a); }
// round(): half away from zero (histogram.cl:28-29; oracle/orc_volume.py _round_half_away)
float cl_round(float a) __asm__("_Z5roundf");
float cl_round(float a) { return roundf(a); }
// reached by no kernel the driver runs (get_random_direction, sample_environment_map_e): defined so that the library links
float cl_atan(float a) __asm__("_Z4atanf");
float cl_atan(float a) { return (float)atan((double)a); }
float cl_sin(float a) __asm__("_Z3sinf");
float cl_sin(float a) { return (float)sin((double)a); }
float cl_cos(float a) __asm__("_Z3cosf");
float cl_cos(float a) { return (float)cos((double)a); }
float cl_ldexp(float a, int e) __asm__("_Z5ldexpfi");
float cl_ldexp(float a, int e) { return ldexpf(a, e); }

// ---- the compiled reference (and oracle/ref/ref_cl_driver.cl), as the OpenCL object exports it ------------------------------
struct ray { float3 origin, direction; };
struct cut_result { bool cut; float3 cut_point; };
unsigned hash(unsigned seed);
struct ray generate_ray(struct ray camera, int x, int y, int x_total, int y_total);
struct cut_result cut(image_t reference_volume, struct ray shot);
void render(image_t frame, image_t volume, image_t sdf, image_t env, uint16_t *buffer_volume, float px, float py, float pz,
            float dx, float dy, float dz, int seed);
void ref_driver_render_ao(image_t frame, image_t volume, image_t sdf, uint16_t *buffer_volume, uint32_t *shade, int launch_w,
                          float px, float py, float pz, float dx, float dy, float dz, int seed);
void bilateral_filter(image_t volume, image_t out);
void fetch_stats(image_t volume, int32_t *stats);
void apply_clip(image_t original, image_t clipped, uint32_t *start, uint32_t *end);
void tf_sort_values(image_t volume, uint32_t *frame, int width, int height, float min_v, float max_v, float min_g, float max_g);
void buffer_reset(image_t volume, uint16_t *buffer_volume);

}  // extern "C"

// ---- (b) the driver ---------------------------------------------------------------------------------------------------------
namespace {

int g_abi_status = -1;

// hash: utility_sampling.cl:13-21 by hand (tests/test_oracle_render.py test_hash_known_answers' inputs); cut: the three cases of
// test_cut_literal_semantics; generate_ray: a camera along +z, whose side / up vectors are the x / y axes exactly
int abi_self_check() {
  const unsigned in[5] = {0u, 1u, 0xFFFFFFFFu, 1804289383u, 0x182205BDu};
  for (unsigned s : in) {
    unsigned v = (s ^ 61u) ^ (s >> 16);
    v <<= 3; v ^= v >> 4; v *= 0xDEADBEEFu; v ^= v >> 15;
    if (hash(s) != v) return 1;
  }
  int16_t voxels[1] = {0};
  image vol = {10, 10, 10, ELEM_I16, voxels};
  struct ray shot;
  shot.origin = (float3){-5.0f, 5.0f, 5.0f};
  shot.direction = (float3){1.0f, 0.0f, 0.0f};
  struct cut_result c = cut(&vol, shot);
  if (!c.cut || c.cut_point.x != 0.0f || c.cut_point.y != 5.0f || c.cut_point.z != 5.0f) return 2;
  shot.direction = (float3){-1.0f, 0.0f, 0.0f};
  c = cut(&vol, shot);
  if (!c.cut || c.cut_point.x != -5.0f || c.cut_point.y != 5.0f || c.cut_point.z != 5.0f) return 3;
  shot.origin = (float3){-5.0f, 20.0f, 30.0f};
  c = cut(&vol, shot);
  if (c.cut) return 4;
  struct ray cam;
  cam.origin = (float3){1.0f, 2.0f, 3.0f};
  cam.direction = (float3){0.0f, 0.0f, 1.0f};
  struct ray r = generate_ray(cam, 4, 2, 8, 4);
  if (r.origin.x != 1.0f || r.origin.y != 2.0f || r.origin.z != 3.0f) return 5;
  if (r.direction.x != 0.0f || r.direction.y != 0.0f || r.direction.z != 1.0f) return 6;
  r = generate_ray(cam, 6, 3, 8, 4);  // x_offset = 2/8 * 2 = 0.5, y_offset = 1/4
  const float l = sqrtf((0.5f * 0.5f + 0.25f * 0.25f) + 1.0f);
  if (r.direction.x != 0.5f / l || r.direction.y != 0.25f / l || r.direction.z != 1.0f / l) return 7;
  return 0;
}

__attribute__((constructor)) void abi_check_on_load() {
  g_abi_status = abi_self_check();
  if (g_abi_status) fprintf(stderr, "libref_cl: ABI self-check failed at step %d; every entry point will refuse to run\n", g_abi_status);
}

void begin(const void *atomic_base, int64_t atomic_words, bool logging) {
  g_atomic_base = static_cast<const int32_t *>(atomic_base);
  g_atomic_words = atomic_words;
  g_logging = logging;
  g_log.clear();
  g_out_of_range = 0;
  g_trace_unexpected = 0;
  memset(g_exit_depth, 0, sizeof g_exit_depth);
}

template <class F> void launch3(const int32_t g[3], F body) {
  for (int32_t z = 0; z < g[2]; ++z)
    for (int32_t y = 0; y < g[1]; ++y)
      for (int32_t x = 0; x < g[0]; ++x) {
        g_id[0] = (size_t)x; g_id[1] = (size_t)y; g_id[2] = (size_t)z;
        g_gid = x + (int64_t)g[0] * (y + (int64_t)g[1] * z);
        g_path.active = false;
        body();
      }
}

}  // namespace

#define API extern "C" __attribute__((visibility("default")))

API int refcl_abi_status() { return g_abi_status; }
API long long refcl_out_of_range() { return g_out_of_range; }
// of the last refcl_render: paths that ended in Exit_volume after 0, 1, 2 Hits; returns the calls the trace could not place
API long long refcl_exit_depths(long long out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = g_exit_depth[k];
  return g_trace_unexpected;
}

// elem: 0 int8 (the SDF), 1 int16 (the volume), 2 RGBA8 (frame, environment map).  The array is borrowed, not copied.
API void *refcl_image(int w, int h, int d, int elem, void *data) { return new image{w, h, d, elem, data}; }
API void refcl_image_free(void *im) { delete static_cast<image *>(im); }

// One launch of `render` (ray_marching.cl:152-199) over launch_w x launch_h work-items, rows outer, x inner.
// hit_entry[launch_w * launch_h]: the cache entry the pixel's token request addressed, -1 where it made none (no hit);
// contrib[.. * 4]: {r, g, b} of the pixel's atomic_buffer_volume_add4 and 1, zeros where the token was refused.
API int refcl_render(void *frame, void *volume, void *sdf, void *env, uint16_t *cache, long long cache_len, const float *cam_pos,
                     const float *cam_dir, int seed, int launch_w, int launch_h, long long *hit_entry, uint32_t *contrib) {
  if (g_abi_status) return -100;
  image *f = static_cast<image *>(frame);
  if (launch_w > f->w || launch_h > f->h || (cache_len & 1)) return -1;
  const int64_t npx = (int64_t)launch_w * launch_h;
  begin(cache, cache_len / 2, true);
  const int32_t g[3] = {launch_w, launch_h, 1};
  launch3(g, [&] {
    render(f, static_cast<image *>(volume), static_cast<image *>(sdf), static_cast<image *>(env), cache, cam_pos[0], cam_pos[1],
           cam_pos[2], cam_dir[0], cam_dir[1], cam_dir[2], seed);
  });
  for (int64_t i = 0; i < npx; ++i) hit_entry[i] = -1;
  memset(contrib, 0, (size_t)npx * 4 * sizeof(uint32_t));
  // per work-item the log is: token request (word 2e+1, +0x10000), then either its return (-0x10000) or the two adds
  size_t k = 0;
  while (k < g_log.size()) {
    const int64_t gid = g_log[k].gid;
    size_t n = k;
    while (n < g_log.size() && g_log[n].gid == gid) ++n;
    const atomic_record *r = &g_log[k];
    if (r[0].addend != 0x00010000 || !(r[0].word & 1)) return -2;
    const int64_t e = r[0].word / 2;
    hit_entry[gid] = e;
    if (n - k == 2) {
      if (r[1].word != r[0].word || r[1].addend != -0x00010000) return -3;
    } else if (n - k == 3) {
      if (r[1].word != 2 * e || r[2].word != 2 * e + 1) return -4;
      const uint32_t low = (uint32_t)r[1].addend, high = (uint32_t)r[2].addend;
      uint32_t *c = contrib + gid * 4;
      c[0] = low & 0xFFFFu; c[1] = low >> 16; c[2] = high & 0xFFFFu; c[3] = 1u;
      if (high >> 16) return -5;  // the count travels through the token, never through the add
    } else {
      return -6;
    }
    k = n;
  }
  return g_out_of_range ? -7 : 0;
}

// One launch of ref_driver_render_ao (oracle/ref/ref_cl_driver.cl): compute_ao for every work-item; shade[launch_w * launch_h] gets
// the .x of what compute_ao returned.  `cache_len` counts ushorts of the 2-channel view.
API int refcl_render_ao(void *frame, void *volume, void *sdf, uint16_t *cache, long long cache_len, const float *cam_pos,
                        const float *cam_dir, int seed, int launch_w, int launch_h, uint32_t *shade) {
  if (g_abi_status) return -100;
  image *f = static_cast<image *>(frame);
  if (launch_w > f->w || launch_h > f->h) return -1;
  (void)cache_len;
  begin(nullptr, 0, false);
  const int32_t g[3] = {launch_w, launch_h, 1};
  launch3(g, [&] {
    ref_driver_render_ao(f, static_cast<image *>(volume), static_cast<image *>(sdf), cache, shade, launch_w, cam_pos[0], cam_pos[1],
                         cam_pos[2], cam_dir[0], cam_dir[1], cam_dir[2], seed);
  });
  return 0;
}

// The pre-processing kernels over a 3-D global size, z outer, x inner.
API int refcl_bilateral_filter(void *volume, void *out, const int32_t *global) {
  if (g_abi_status) return -100;
  begin(nullptr, 0, false);
  launch3(global, [&] { bilateral_filter(static_cast<image *>(volume), static_cast<image *>(out)); });
  return g_out_of_range ? -7 : 0;
}
API int refcl_fetch_stats(void *volume, int32_t *stats5, const int32_t *global) {
  if (g_abi_status) return -100;
  begin(stats5, 5, false);
  launch3(global, [&] { fetch_stats(static_cast<image *>(volume), stats5); });
  return g_out_of_range ? -7 : 0;
}
API int refcl_apply_clip(void *original, void *clipped, uint32_t *start, uint32_t *end, const int32_t *global) {
  if (g_abi_status) return -100;
  begin(nullptr, 0, false);
  launch3(global, [&] { apply_clip(static_cast<image *>(original), static_cast<image *>(clipped), start, end); });
  return g_out_of_range ? -7 : 0;
}
// bins outside width * height are dropped and counted (the reference writes out of bounds for them); returns that count
API long long refcl_tf_sort_values(void *volume, uint32_t *frame, int width, int height, float min_v, float max_v, float min_g,
                                   float max_g, const int32_t *global) {
  if (g_abi_status) return -100;
  begin(frame, (int64_t)width * height, false);
  launch3(global, [&] { tf_sort_values(static_cast<image *>(volume), frame, width, height, min_v, max_v, min_g, max_g); });
  return g_out_of_range;
}
API int refcl_buffer_reset(void *volume, uint16_t *cache, const int32_t *global) {
  if (g_abi_status) return -100;
  begin(nullptr, 0, false);
  launch3(global, [&] { buffer_reset(static_cast<image *>(volume), cache); });
  return 0;
}
