"""Compiles a C twin (tests/*_twin.c) on first use with the system compiler and -O2 -ffp-contract=off (no product fused into a sum) and loads it with ctypes.  The shared
object is cached in a per-user temporary directory under a name that carries the hash of the .c file and of every local header it includes, so an edit to any of them
builds anew."""
import ctypes
import hashlib
import os
import re
import subprocess
import tempfile

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = re.compile(rb'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def sources(path):
    """the file and every file it includes with #include "...", transitively, in the order met"""
    out, todo = [], [os.path.abspath(path)]
    while todo:
        p = todo.pop(0)
        if p in out:
            continue
        out.append(p)
        todo += [os.path.normpath(os.path.join(os.path.dirname(p), m.decode())) for m in _INCLUDE.findall(open(p, "rb").read())]
    return out


def key(path):
    h = hashlib.sha1()
    for p in sources(path):
        h.update(open(p, "rb").read())
    return h.hexdigest()[:12]


def load(c_file_name):
    """c_file_name: a file of this directory, or a path"""
    src = os.path.join(_HERE, c_file_name)
    d = os.path.join(tempfile.gettempdir(), "dvbs2_twins_%d" % os.getuid())
    os.makedirs(d, exist_ok=True)
    so = os.path.join(d, "%s_%s.so" % (os.path.splitext(os.path.basename(src))[0], key(src)))
    if not os.path.exists(so):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, src, "-lm"])
        os.replace(tmp, so)
    return ctypes.CDLL(so)
