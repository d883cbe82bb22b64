"""uchirp._binding -- the one ctypes loader behind the sibling libraries' modules (link, scene, array, align, xcorr, retime,
track, rate): where libuchirp_<name>.so lies, how it is built, how it is loaded into a process that torch may share, and how a
negative return code becomes the module's exception.  A module keeps its public names by taking them from its Binding
    _so = Binding("align", AlignError, _declare, env="UCHIRP_ALIGN_LIB")
    LIB_PATH, build, lib, _check = _so.path, _so.build, _so.lib, _so.check
and writes only `_declare(L)`: the argtypes of its own entry points."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # ultrasonic-communication_amd/


class Binding:
    def __init__(self, name, error, declare, env=None):
        """`error`: the module's exception class; `declare(L)`: sets the argtypes of what is the module's own (create
        included); `env`: the environment variable that names a diagnostic build to load instead, if the module has one."""
        self.prefix = "uc_%s_" % name
        self.so = "libuchirp_%s.so" % name
        self.error, self.declare, self.env = error, declare, env
        self.path = (env and os.environ.get(env)) or os.path.join(ROOT, self.so)
        self._lib = None

    def build(self, force=False):
        """Compile the library for gfx950 with hipcc (in-tree)."""
        if self.env and os.environ.get(self.env):    # a diagnostic build named by the caller: it is what it is
            return self.path
        if force or not os.path.exists(self.path):
            subprocess.check_call(["make", "-C", ROOT] + (["-B"] if force else []) + [self.so])
        else:
            subprocess.check_call(["make", "-C", ROOT, self.so], stdout=subprocess.DEVNULL)
        return self.path

    def lib(self):
        """Load the library; raises the module's exception if it is absent (no fallback)."""
        if self._lib is not None:
            return self._lib
        # one process, ONE HIP runtime: torch's bundled libamdhip64 first (see uchirp.lib())
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(self.path):
            raise self.error("%s not built: run `make -C %s %s` (hipcc, gfx950); there is no CPU fallback" % (self.so, ROOT, self.so))
        L = C.CDLL(self.path)
        getattr(L, self.prefix + "abi_version").restype = C.c_int
        getattr(L, self.prefix + "last_error").restype = C.c_char_p
        destroy = getattr(L, self.prefix + "destroy")
        destroy.argtypes, destroy.restype = [C.c_void_p], None
        self.declare(L)
        self._lib = L
        return L

    def check(self, rc, what):
        if rc < 0:
            msg = getattr(self.lib(), self.prefix + "last_error")()
            raise self.error("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))
        return rc
