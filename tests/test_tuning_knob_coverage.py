"""Every environment variable the library reads is accounted for: a tuning variable must be named by tests/test_gpu_tuning_knobs.py, a
switch that another module covers is listed here with that module, and so is the environment's spelling of an option that the suite sets
through rtgl_set_option.  A new getenv("RTGL_AMD_...") in rtgl_amd.hip, or a new environment name in the option table (rt_options.hpp),
fails this test until it is put in one of the lists -- or tested."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

# switches with a test module of their own
COVERED_ELSEWHERE = {
    "RTGL_AMD_CULL_NODE": "test_gpu_cull_nodes.py",
    "RTGL_AMD_SORT_MOVE": "test_gpu_bin_gather.py",
    "RTGL_AMD_NO_CAMERA_KEEP": "test_gpu_parity.py",
    "RTGL_AMD_ALLOW_CONCURRENT_PIPELINES": "test_gpu_torch_plumbing.py",
    "RTGL_AMD_FRAME_BATCH": "test_facade.py",
    "RTGL_AMD_MULTI_THREADS": "test_gpu_fullsize.py",
}
# the environment's spelling of a context option: (option, a module that sets it)
OPTION_SPELLINGS = {
    "RTGL_AMD_KERNEL": ("kernel", "test_gpu_scene_fuzz.py"),
    "RTGL_AMD_SCAN_WAVES": ("scan_waves", "test_gpu_tuning_knobs.py"),
    "RTGL_AMD_SCAN_DYNAMIC": ("scan_dynamic", "test_gpu_tuning_knobs.py"),
    "RTGL_AMD_NARROW_FUSED": ("narrow_fused", None),
    "RTGL_AMD_CAMERA_LEAN": ("camera_lean", None),
    "RTGL_AMD_SHADE_PASS": ("shade_pass", None),
}
# no kernel path: who owns the HIP streams of concurrent pipelines
NOT_A_KERNEL_PATH = {"RTGL_AMD_PRIVATE_STREAMS"}
# debugging aids, not tuning: named RTGL_DEBUG_*
DEBUG = {"RTGL_DEBUG_CAND_CAP": "test_gpu_mfma_edges.py"}


def read(path):
    with open(path) as f:
        return f.read()


def test_every_variable_the_library_reads_is_tested_or_listed():
    code = read(os.path.join(ROOT, "raytracer.glsl_amd", "csrc", "rtgl_amd.hip"))
    for name in os.listdir(os.path.join(ROOT, "raytracer.glsl_amd", "csrc")):
        if name.endswith(".hpp"):
            assert "getenv(" not in read(os.path.join(ROOT, "raytracer.glsl_amd", "csrc", name)), f"{name} reads the environment"
    # ... so the spellings of the options are names in the option table (rt_options.hpp), which rtgl_amd.hip reads through its own getter
    spellings = set(re.findall(r'"(RTGL_[A-Z_]+)"', read(os.path.join(ROOT, "raytracer.glsl_amd", "csrc", "rt_options.hpp"))))
    assert spellings == set(OPTION_SPELLINGS) | {"RTGL_AMD_SORT_MOVE", "RTGL_AMD_FRAME_BATCH"} and "rt_options::read_environment(ctx->opt," in code
    names = set(re.findall(r'getenv\("(RTGL_[A-Z_]+)"\)', code))
    assert not names & spellings
    names |= spellings
    assert len(names) == 24      # what the getenv calls of rtgl_amd.hip alone named before the table
    knobs = read(os.path.join(TESTS, "test_gpu_tuning_knobs.py"))
    listed = set(COVERED_ELSEWHERE) | set(OPTION_SPELLINGS) | NOT_A_KERNEL_PATH | set(DEBUG)
    missing = sorted(n for n in names - listed if n not in knobs)
    assert not missing, f"read by rtgl_amd.hip, named neither by tests/test_gpu_tuning_knobs.py nor by the lists of this test: {missing}"
    assert not (listed - names), f"listed here but no longer read: {sorted(listed - names)}"
    # the ten variables of the device module, by name
    for n in ("HYBRID_DIV", "SORT_OB", "SORT_DB", "BIN_SPLIT", "BIN_UNIT", "ITEMS_PER_WAVE", "KD_LAMBDA", "ROW_GAMMA", "SCHED_FILL", "HIST_FILL"):
        assert "RTGL_AMD_" + n in names and len(re.findall("RTGL_AMD_" + n, knobs)) >= 2, n      # (the docstring's list and a test)


def test_the_lists_point_at_tests_that_exist():
    for name, module in list(COVERED_ELSEWHERE.items()) + list(DEBUG.items()):
        assert name in read(os.path.join(TESTS, module)), (name, module)
    every = {f: read(os.path.join(TESTS, f)) for f in os.listdir(TESTS) if f.endswith(".py")}
    for name, (option, module) in OPTION_SPELLINGS.items():
        users = [f for f, text in every.items() if re.search(r'"%s"' % option, text) and f != os.path.basename(__file__)]
        assert users, f"no test sets option {option} ({name})"
        if module:
            assert module in users, (name, module, users)
