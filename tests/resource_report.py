"""The compiler's resource remarks of every kernel, shared by the modules that pin them (no GPU needed: hipcc cross-compiles)."""
import functools
import os
import re
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer.glsl_amd", "csrc")


@functools.lru_cache(maxsize=None)
def report():
    """{mangled kernel name: {remark: number}} from `make -B asm`: a device-only compile of the library's one translation unit, minutes
    long, so it runs once per process; it rewrites the ignored csrc/rtgl_amd.gfx950.s and nothing else.  Read it, do not change it."""
    out = subprocess.run(["make", "-B", "-C", CSRC, "asm"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rep, cur = {}, None
    for line in (out.stdout + out.stderr).splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rep[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\d+)", line)
        if m and cur:
            rep[cur][m.group(1).strip()] = int(m.group(2))
    return rep
