"""The one builder of the host-built TEST AIDS (tests/hostsim, hostsim_gi, hostsim_path, hostsim_plant, hostsim_trace):
the compiler command line, the rebuild rule, the replace step and the rendered arm-table header.  Each aid keeps its
sources, its -D flags, its ctypes signatures and its cache of loaded libraries.  Never imported by the product."""
import hashlib
import os
import subprocess

from abr_control_amd import _abi

_TESTS = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_TESTS, "..", "abr_control_amd", "csrc")
ABRK_H = os.path.join(_TESTS, "..", "include", "abrk.h")
# -fno-signed-zeros -ffinite-math-only must equal MATHFLAGS of abr_control_amd/csrc/Makefile: with them the host build
# has the roundings of a GPU lane
HOST_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-signed-zeros",
              "-ffinite-math-only", "--cuda-host-only"]


def csrc(*names):
    """paths of headers under abr_control_amd/csrc"""
    return [os.path.join(_CSRC, n) for n in names]


def command(src, out, defs=()):
    return ["/opt/rocm/bin/hipcc", *HOST_FLAGS, *defs, "-o", out, src]


def stale(src, out, deps):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in [src, *deps])


def _aid(src):
    return os.path.splitext(os.path.basename(src))[0]


def build_many(src, deps, outs_defs, force=False):
    """the libraries {out: defs} of one source, the stale ones compiled side by side; each appears under its name
    complete or not at all"""
    procs = []
    for out, defs in outs_defs.items():
        if force or stale(src, out, deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            tmp = f"{out}.{os.getpid()}.tmp"
            procs.append((out, tmp, subprocess.Popen(command(src, tmp, defs), stdout=subprocess.DEVNULL,
                                                     stderr=subprocess.PIPE, text=True)))
    errors = []
    for out, tmp, p in procs:
        err = p.communicate()[1]
        if p.returncode:
            errors.append(err)
            if os.path.exists(tmp):
                os.remove(tmp)
        else:
            os.replace(tmp, out)
    if errors:
        raise RuntimeError(f"{_aid(src)} build failed:\n" + errors[0][-3000:])


def build(src, out, deps, defs=()):
    """compile `src` into `out` when `out` is missing or older than `src` or one of `deps`"""
    build_many(src, deps, {out: defs})
    return out


def table_header(build_dir, table, struct_name):
    """`table` rendered as the compile-time struct abrk::<struct_name> in a header under build_dir (written once: its
    name carries the hash of its text) -> (key, header path)"""
    text = _abi.render_tab_struct(table, struct_name)
    key = hashlib.sha256(text.encode()).hexdigest()[:16]
    hdr = os.path.join(build_dir, f"tab_{key}.h")
    if not os.path.exists(hdr):
        os.makedirs(build_dir, exist_ok=True)
        tmp = f"{hdr}.{os.getpid()}.tmp"
        with open(tmp, "w") as fh:
            fh.write("#pragma once\nnamespace abrk {\n" + text + "\n}  // namespace abrk\n")
        os.replace(tmp, hdr)
    return key, hdr
