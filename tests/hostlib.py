"""One way to build a host-check library: the pattern rules of
tests/hostcheck/Makefile (source stem -> lib<stem>.so or the program <stem>,
the g++ flags stated there once), run into a directory of the caller's."""
import ctypes as C
import os
import subprocess

HOSTCHECK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcheck")


def make(out_dir, target):
    """`target` of the hostcheck Makefile built into out_dir; its path."""
    subprocess.run(["make", "-s", "-C", HOSTCHECK, "BUILD=" + str(out_dir), os.path.join(str(out_dir), target)],
                   check=True)
    return os.path.join(str(out_dir), target)


def build(out_dir, stem):
    """tests/hostcheck/<stem>.cpp as a shared library in out_dir, loaded."""
    return C.CDLL(make(out_dir, "lib%s.so" % stem))
