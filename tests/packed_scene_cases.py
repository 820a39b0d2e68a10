"""The inputs of the read-back tests of the derived scene data (tests/test_gpu_packed_scene.py, tests/test_gpu_view_data.py): shapes,
volumes, SDF images and transfer functions.  tests/test_packed_scene_cpu.py asserts, without a GPU, that each of them exercises what
it is here for."""
import numpy as np

from cl_volume_renderer_amd import scene

# k_repack: a block handles 64 x 8 x 8 voxels; its 16-byte staging needs X % 16 == 0 and the block's 64 voxels inside the row
REPACK_SHAPES = [
    (64, 8, 8),      # one block, 16-byte path
    (128, 16, 16),   # 16-byte path with real halo voxels left and right of the seam x = 63 | 64 and between blocks in y and z
    (80, 9, 9),      # 16-byte path in the first block, voxel by voxel in the second; ragged y and z: padding rows
    (16, 8, 8),      # a multiple of 16, shorter than a block
    (72, 40, 56),    # never the 16-byte path
    (144, 24, 40),
    (7, 9, 17), (2, 2, 2), (1, 1, 1),
]
# k_proj_repack: its 16-byte path needs X % 8 == 0
VIEW_SHAPES = [
    (72, 9, 9),      # 16-byte path, the second block holds one brick
    (70, 33, 45),    # voxel by voxel
    (64, 8, 8), (8, 8, 8), (1, 1, 1),
    (40, 40, 136),   # 5 x 5 x 17 bricks: partial cells of 4^3 bricks on every axis, the last layer along z a single brick thick
]
LARGE_SHAPE = (200, 170, 150)   # many blocks in flight
# the shapes on which the gradient table must leave and write a tenth of the sub-bricks each
GRADIENT_SHAPES = [(64, 64, 64), (80, 9, 9), (72, 40, 56)]
RANDOM_SHAPES = [(128, 16, 16), (80, 9, 9), (72, 40, 56), (7, 9, 17)]

# a camera that looks away from every volume of the list: no pixel hits, nothing marches
CAMERA_AWAY = (np.array([-100, 200, -100], np.float32), (np.array([-0.6, 0.5, -0.6]) / np.linalg.norm([-0.6, 0.5, -0.6])).astype(np.float32))

# three rectangles: the first reads `gradient` and stands ahead of two that do not; the windows overlap (30..950 lies in the first's,
# 30..45 in all three), so the first match decides; the first and the third window contain 0
TF_THREE_RECTS = scene.tf_rect_source([(-50.0, 1000.0, 100.0, 4000.0, (1.0, 0.8, 0.6, 0.5)),
                                       (30.0, 950.0, 0.0, 4000.0, (0.2, 0.4, 0.6, 0.8)),
                                       (-30.0, 45.0, 0.0, 4000.0, (0.9, 0.1, 0.3, 1.0))])
# every voxel an event of class 2: no value lies in the first rectangle's window (its bounds are crossed), the second covers the whole range
TF_ALL_CLASS_2 = scene.tf_rect_source([(6000.0, 5000.0, 0.0, 4000.0, (1.0, 0.0, 0.0, 1.0)),
                                       (-32768.0, 32767.0, 0.0, 4000.0, (0.0, 1.0, 0.0, 1.0))])
# outside the rule grammar (an `||`): compiled per context, one colour, so every event has class 1
TF_FREE_FORM = ("inline bool is_event_gen(short value, short gradient, int4 *color){\n"
                "  int4 shade = {229, 153, 76, 178};\n"
                "  if(value >= -100 && value <= 300 || value == 31000) { *color = shade; return true; }\n"
                "  return false;\n}\n")
RULE_TFS = {"default": scene.tf_default_source(), "gradient": scene.tf_gradient_source(), "three_rects": TF_THREE_RECTS,
            "gt800": scene.TF_TEST_VALUE_GT_800}


def free_form_classes(vol):
    """TF_FREE_FORM's event set in numpy"""
    v = np.asarray(vol).astype(np.int32)
    return (((v >= -100) & (v <= 300)) | (v == 31000)).astype(np.uint8)


def phantom(dims):
    return scene.phantom(max(dims), dims=dims)


def free_form_volume(dims):
    """the phantom with a few voxels of the value only the `||` reaches"""
    vol = phantom(dims)
    vol.reshape(-1)[::37] = 31000
    return vol


def random_volume(dims, seed=11):
    """uniform int16 over the whole range; -32768 and 32767 stand next to each other along every axis and next to the faces, so the
    central differences reach +-65535 and +-32768 (border 0), and the tables' keys v + 32768 and 32767 - v reach 0 and 65535"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vol = rng.integers(-32768, 32768, size=(Z, Y, X)).astype(np.int16)
    if min(dims) >= 7:
        cz, cy, cx = Z // 2, Y // 2, X // 2
        for axis in range(3):   # low, centre, high along the axis; the centre voxel's difference is +65535, one further -65535
            for k, v in ((-1, -32768), (1, 32767), (3, -32768)):
                at = [cz, cy, cx]
                at[axis] += k
                vol[tuple(at)] = v
        vol[0, 0, 0], vol[0, 0, 1] = 32767, -32768
        vol[Z - 1, Y - 1, X - 1], vol[Z - 1, Y - 1, X - 2] = -32768, 32767
    return vol


def mixed_volume(dims):
    """the phantom below z = Z / 2, uniform random values above: events, undecided voxels (in a value window, the gradient clause failed)
    and plain ones in numbers, and -- unlike the phantom, whose shell is thinner than a sub-brick -- sub-bricks that are written
    although they hold no event"""
    vol = phantom(dims)
    half = dims[2] // 2
    vol[half:] = random_volume(dims)[half:]
    return vol


def random_sdf(dims, seed=12):
    """uniform int8 over all 256 values: negative values, 0, 1 (below the certificates' smallest step) and 127 all occur"""
    X, Y, Z = dims
    sdf = np.random.default_rng(seed).integers(-128, 128, size=(Z, Y, X)).astype(np.int8)
    if sdf.size >= 256:
        sdf.reshape(-1)[:256] = np.arange(-128, 128).astype(np.int8)
    return sdf


def swapped(vol):
    """air and ball swapped: what was air becomes dense, everything else air"""
    return np.where(np.asarray(vol) < -500, 900, -1000).astype(np.int16)
