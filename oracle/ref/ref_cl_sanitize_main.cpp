// oracle/ref/ref_cl_sanitize_main.cpp -- TEST INFRASTRUCTURE ONLY.  A stand-alone program for `make -C oracle/ref sanitize`: the
// shim and the compiled reference kernels under -fsanitize=address,undefined,float-cast-overflow on a scene made right here
// (a shell of 900 in -1000, SDF 0 everywhere -- every step 0.5 --, a gradient sky), camera outside, inside and edge-on, the
// light passes and compute_ao.  float-cast-overflow is the check for the float -> integer conversions OpenCL C leaves
// undefined: any report ends the program.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int refcl_abi_status();
void *refcl_image(int w, int h, int d, int elem, void *data);
void refcl_image_free(void *im);
int refcl_render(void *frame, void *volume, void *sdf, void *env, uint16_t *cache, long long cache_len, const float *cam_pos,
                 const float *cam_dir, int seed, int launch_w, int launch_h, long long *hit_entry, uint32_t *contrib);
int refcl_render_ao(void *frame, void *volume, void *sdf, uint16_t *cache, long long cache_len, const float *cam_pos,
                    const float *cam_dir, int seed, int launch_w, int launch_h, uint32_t *shade);
}

int main() {
  const int X = 20, Y = 28, Z = 17, W = 96, H = 64, EW = 64, EH = 32;
  std::vector<int16_t> vol((size_t)X * Y * Z);
  std::vector<int8_t> sdf(vol.size(), 0);
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const float r = std::sqrt((x - 9.5f) * (x - 9.5f) + (y - 13.5f) * (y - 13.5f) + (z - 8.0f) * (z - 8.0f));
        vol[((size_t)z * Y + y) * X + x] = (int16_t)((r > 5.0f && r < 7.5f && x != 9) ? 900 + (x * 7 + y * 3 + z) % 40 : -1000);
      }
  std::vector<uint8_t> env((size_t)EW * EH * 4), frame((size_t)W * H * 4);
  for (size_t i = 0; i < env.size(); ++i) env[i] = (uint8_t)(40 + (i * 37) % 200);
  std::vector<uint16_t> cache(((size_t)X * Z * Y + (size_t)X * Z + X + 1) * 4);
  std::vector<long long> hit((size_t)W * H);
  std::vector<uint32_t> contrib((size_t)W * H * 4), shade((size_t)W * H);
  void *fi = refcl_image(W, H, 1, 2, frame.data()), *vi = refcl_image(X, Y, Z, 1, vol.data()), *si = refcl_image(X, Y, Z, 0, sdf.data()),
       *ei = refcl_image(EW, EH, 1, 2, env.data());
  if (refcl_abi_status()) return 1;
  const float poses[3][3] = {{-9.0f, 20.0f, -9.0f}, {4.0f, 20.0f, 5.0f}, {28.0f, 36.0f, 8.5f}};
  long long hits = 0, granted = 0;
  for (const auto &p : poses) {
    float d[3] = {10.0f - p[0], 14.0f - p[1], 8.5f - p[2]};
    const float l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (float &c : d) c /= l;
    for (int seed = 1; seed <= 6; ++seed) {
      if (refcl_render(fi, vi, si, ei, cache.data(), (long long)cache.size(), p, d, (int)((unsigned)seed * 1804289383u), W, H, hit.data(), contrib.data())) return 2;
      for (size_t i = 0; i < hit.size(); ++i) { hits += hit[i] >= 0; granted += contrib[i * 4 + 3]; }
    }
    for (auto &c : cache) c = 0;
    for (int seed = 1; seed <= 6; ++seed)
      if (refcl_render_ao(fi, vi, si, cache.data(), (long long)cache.size(), p, d, (int)((unsigned)seed * 846930886u), W, H, shade.data())) return 3;
    for (auto &c : cache) c = 0;
  }
  for (void *im : {fi, vi, si, ei}) refcl_image_free(im);
  std::printf("sanitize ok: %lld hit samples, %lld granted\n", hits, granted);
  return hits > 1000 && granted > 1000 ? 0 : 4;
}
