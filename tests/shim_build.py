"""The one compiler command line of the suite: a C or C++ program against include/ and the in-tree library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "aswstereomatch_amd")
HEAD = {"c++": ["g++", "-std=c++17", "-Wall"], "c": ["gcc", "-std=c99", "-Wall"]}
C99 = {"lang": "c", "extra": ("-Wextra", "-pedantic")}  # the plain-C boundary: build_demo(src, exe, **C99)


def build_demo(source_name, exe, cv=False, lang="c++", extra=(), link=True):
    """Compile tests/cpp/<source_name> (or an absolute path) to `exe` and return `exe`.  cv: the header's cv::Mat branch against
    tests/cpp/cv_stub, the compile-only stand-in for the OpenCV declarations the header names.  link=False: a program that supplies
    the library's symbols itself."""
    from aswstereomatch_amd import build

    if link and not os.path.exists(build.LIB):
        build.build()
    cmd = HEAD[lang] + list(extra)
    if cv:
        cmd += ["-Wextra", "-DASW_WITH_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "cv_stub")]
    cmd += ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", str(source_name))]
    if link:
        cmd += ["-L" + PKG, "-lasw_mi355x", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    cmd += ["-o", str(exe)]
    subprocess.check_call(cmd)
    return str(exe)
