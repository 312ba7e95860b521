"""The C side of the ABI tests: the one layout probe that holds ctypes mirrors to include/gops_hip.h, and what every `test_abi_of_*`
asks of its entry points."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


def layout_probe(tmp_path, structs, c_names=None):
    """One C99 program against the header (plain C: the boundary is a C ABI) prints sizeof of every struct and offsetof of every
    member; the ctypes classes are held to it - a field added on one side only, or moved into what used to be padding, fails here.
    `structs`: (C struct name, ctypes class), or (C struct name, size) for a struct without a mirror; `c_names`: a ctypes field
    name -> its C spelling where the two differ."""
    c_names = c_names or {}
    lines, want = [], []
    for st, cls in structs:
        lines.append(f'    printf(" %zu", sizeof({st}));\n')
        if isinstance(cls, int):
            want.append((st, cls))
            continue
        lines += [f'    printf(" %zu", offsetof({st}, {c_names.get(f[0], f[0])}));\n' for f in cls._fields_]
        want += [(st, ctypes.sizeof(cls))] + [(f"{st}.{f[0]}", getattr(cls, f[0]).offset) for f in cls._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gops_hip.h"\nint main(void) {\n' + "".join(lines) + "    return 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert len(got) == len(want)
    differ = [(what, g, w) for (what, w), g in zip(want, got) if g != w]
    assert not differ, differ   # (what, the header's value, the mirror's)


def check_abi(tmp_path, structs, entry_points, stats):
    """The entry points are declared in the header (plain C99), exported by the library and listed by hip_backend; the version stays
    15; `stats`: (macro, hip_backend's value); `structs`: as `layout_probe` takes them."""
    from gops_amd import hip_backend as hb
    header = open(os.path.join(INCLUDE, "gops_hip.h")).read()
    assert "#define GOPS_HIP_ABI_VERSION 15" in header
    for name in entry_points:
        assert re.search(rf"\b{name}\s*\(", header) and name in hb.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(hb.LIB_PATH), name)
    for macro, value in stats:
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value
    layout_probe(tmp_path, structs)
