// oracle/ref/ref_cl_driver.cl -- TEST INFRASTRUCTURE ONLY, our own text; oracle/ref/Makefile appends it to the translation
// unit made of the reference's kernels.  No kernel of the reference reaches compute_ao (ray_marching.cl:104-149; render calls
// compute_light), so this entry calls the reference's generate_ray, in_volume, cut and compute_ao the way render calls
// compute_light, and hands back the .x of compute_ao's result per work-item (0 where the primary ray misses).

// The reference declares these `inline` only; in C99 that is an inline definition without an external one, and a call the
// optimiser does not inline stays undefined.  One declaration without `inline` makes the definition above external.
float4 make_float4(float3 value, float other);
float4 make_float(int4 in);
int4 make_int(float4 value);
bool allow_write_max(int3 refdimensions, __global unsigned short *buffer_volume, int4 pos, unsigned int max);
struct line_cut_result cut_min_eval(float a, float b);
bool exited_volume(__read_only image3d_t reference_volume, float4 position);
enum event get_event_and_value(__read_only image3d_t reference_volume, float4 position, int4 *value_at_event);
enum event get_event(__read_only image3d_t reference_volume, float4 position);
bool is_event_gen(short value, short gradient, int4 *color);

__kernel void ref_driver_render_ao(__write_only image2d_t frame, __read_only image3d_t reference_volume, __read_only image3d_t sdf,
                                   __global unsigned short *buffer_volume, __global uint *shade, int launch_w, float cam_pos_x,
                                   float cam_pos_y, float cam_pos_z, float cam_dir_x, float cam_dir_y, float cam_dir_z, int random_seed) {
  unsigned int x = get_global_id(0);
  unsigned int y = get_global_id(1);
  struct ray camera = {{cam_pos_x, cam_pos_y, cam_pos_z}, {cam_dir_x, cam_dir_y, cam_dir_z}};
  struct ray vray = generate_ray(camera, x, y, get_image_width(frame), get_image_height(frame));
  struct cut_result where;
  if (in_volume(reference_volume, vray.origin) == false)
    where = cut(reference_volume, vray);
  else {
    struct cut_result res = {true, vray.origin};
    where = res;
  }
  shade[y * launch_w + x] = 0;
  if (!where.cut) return;
  struct ray surface_ray = {where.cut_point, vray.direction};
  uint4 f = compute_ao(surface_ray, reference_volume, sdf, buffer_volume, random_seed);
  shade[y * launch_w + x] = f.x;
}
