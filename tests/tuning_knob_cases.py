"""The shapes of tests/test_gpu_tuning_knobs.py that exist to make the waves of the hybrid scan take several turns and then claim, as
plain data: tests/test_scan_items.py recomputes their launch figures through rt_scan_launch.hpp on the CPU and fails when a change of the
launch policy leaves a family without a wave of two turns.  (Test infrastructure only.)"""

N_CUS = 256                                      # MI355X
HYBRID_DIVS = (1, 2, 3, 4, 7, 64)                # RTGL_AMD_HYBRID_DIV
SCAN_WAVES = (1, 2)                              # option "scan_waves": 4 or 8 waves per block

# family "chunks": more chunks than CUs -- 11,200 triangles = 280 quads, one quad per group and per chunk: one block per chunk, step 4 or 8.
# (width, height) -> granules of 128 rays on the camera bounce; 40 x 40 and 56 x 56 end in a half-full granule
CHUNKS_MESH = (100, 56)                          # scenes.scene_mesh(nx, ny): 2 nx ny triangles
CHUNKS_QUADS = 280
CHUNKS_SIZES = {(48, 32): 12, (40, 40): 13, (56, 56): 25, (80, 64): 40}

# family "blocks": golden_cases.scene_two_meshes (460 triangle visits = 12 quads) at one quad per chunk: 21 blocks per chunk, laid out by
# XCD, step 84 or 168, at a size above waves x CUs / chunks granules
BLOCKS_QUADS = 12
BLOCKS_SIZES = {(256, 176): 352}

# RTGL_AMD_ITEMS_PER_WAVE: 7,000 triangles = 175 quads at the default chunk size of 32 quads, 352 granules: the values cut the mesh differently
ITEMS_PER_WAVE = (1, 2, 8, 1000)
ITEMS_MESH = (70, 50)
ITEMS_QUADS = 175
ITEMS_SIZE = (256, 176)
ITEMS_CHUNK_QUADS = {1: 32, 2: 8, 8: 4, 1000: 4}      # the camera bounce's chunk size per value, by rt_scan_launch::launch


def rays(width, height):
    """the rays of a frame: the 8 x 8-aligned footprint"""
    return (width // 8 * 8) * (height // 8 * 8)


def hybrid_figures(n_gran, step, hybrid_div):
    """(turns of the busiest wave, n_tail) -- rt_scan_items.hpp: n_tail = n_gran / hdiv, the turns are dealt with stride `step`"""
    hdiv = max(hybrid_div, 1)
    n_tail = n_gran // hdiv
    n_turns = n_gran - n_tail
    return (n_turns + step - 1) // step, n_tail
