"""The layout of include/gipuma_hip.h's structs as the C compiler sees it, for the tests that hold a ctypes class against
it: a tiny C program prints sizeof and every offsetof."""
import ctypes as C
import os
import subprocess
import tempfile

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gipuma_hip.h")


def c_layout(structs):
    """{C struct name: field names} -> {name: sizeof, "name.field": offsetof}"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void){']
    for s, fs in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in fs]
    lines.append('return 0;}')
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-o", exe, src])
        out = subprocess.check_output([exe]).decode()
    return {k: int(v) for k, v in (l.split() for l in out.split("\n") if l)}


def assert_mirrors_header(py, name, fields=None):
    """the ctypes class `py` has the size and every field offset of the header's struct `name`; with `fields`, the header's
    field names written out in order, also those names in that order"""
    if fields is None:
        fields = [f for f, _ in py._fields_]
    else:
        assert [f for f, _ in py._fields_] == fields, name
    got = c_layout({name: fields})
    assert got[name] == C.sizeof(py), name
    for f in fields:
        assert got["%s.%s" % (name, f)] == getattr(py, f).offset, (name, f)
