#!/usr/bin/env python3
"""Mutation audit of the storage kernels on the CPU emulation (no GPU is ever used).

Every entry of tools/mutation_audit.json is one small change of a product source ("mutant"):
    id          number in the record (profiles/mutation_audit.md)
    file        source file, relative to the repository root
    find        exact text; must occur exactly `count` times, or the mutant is refused
    replace     what every occurrence becomes
    count       expected occurrences
    tests       test modules that are to notice the change
    what        one line for the report
    equivalent  (optional) why no test can notice: the mutant computes the same thing
    gpu_only    (optional) the -m gpu tests that notice it where no CPU test can; reported apart, never run here
    open        (optional) why no test, on the CPU or on the GPU, is known to notice it although it is a real fault;
                reported apart as OPEN, and stale once a test kills it

Per mutant the tool copies the tree to a throw-away directory, applies the change there, builds the emulation library
(the units of tests/conftest.py with its flags), runs the named modules with -m "not gpu" -- without the sanitizer
harnesses and the hipcc resource gates, which look at other builds -- and prints `killed` with the failing test ids or
`survived`.  The working tree is never touched and nothing is loaded on a device.

The emulation is twelve compilation units and a mutant changes one or two of them: the unmutated tree is compiled once,
`clang++ -MM` says which units read which file, and a mutant recompiles only the units that read its file and links them
with the other objects.  The copy's tests get that library through one fixture appended to the COPY's tests/conftest.py
(a later definition of `emulated_kernels_so` that returns the path, and ra_amd.engine bound to the same library for the
host-only entry points that tests call directly); the repository's conftest is not changed.

Exit status 0: every mutant is killed, or explained (`equivalent`, at most a quarter of the list), `gpu_only` or `open`.

usage: python tools/mutation_audit.py [--tree DIR] [--only ID[,ID...]] [--jobs N] [--stop-at-first]
                                      [--subst OLD=NEW] [--json OUT]
  --tree DIR       audit this tree instead of the one the tool lies in (an unpacked earlier commit, say)
  --subst OLD=NEW  rewrite the find / replace texts first (a tree from before a rename)"""
import argparse
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
SKIP_DIRS = {".git", "profiles", "__pycache__", ".pytest_cache", "build", "_ref"}
SKIP_EXT = (".so", ".o", ".a", ".pyc", ".hsaco", ".co")
DESELECT = "not sanitizers and not scratch and not resources"
FIXTURE = '''

# appended by tools/mutation_audit.py, in its throw-away copy only: the library the tool has linked
@pytest.fixture(scope="session")
def emulated_kernels_so():
    return os.environ["RGB_AUDIT_EMU_SO"]


# ... and the host-only entry points that tests call without a fixture (wal_layout, wal_scan, the bounds) are the mutant's
from ra_amd import engine as _audited_engine
_audited_engine.LIB_PATH = os.environ["RGB_AUDIT_EMU_SO"]
'''


def clang():
    c = shutil.which("clang++", path="/opt/rocm/lib/llvm/bin") or shutil.which("clang++")
    if c is None:
        sys.exit("no clang++ (the emulation build needs __builtin_nontemporal_*)")
    return c


def units():
    u = [("api", "api_on_cpu.cpp", []), ("wal", "wal_on_cpu.cpp", []), ("comm", "comm_on_cpu.cpp", []),
         ("dispatch", "kernel_dispatch_on_cpu.cpp", [])]
    return u + [("kernel_N%d" % n, "kernel_on_cpu.cpp", ["-DRGB_EMU_ONLY_N=%d" % n]) for n in range(1, 9)]


def flags(tree):
    nat = os.path.join(tree, "tests", "native")
    return ["-std=c++17", "-O1", "-fPIC", "-DRGB_EMU_FULL_API", "-Wno-unknown-pragmas", "-Wno-pass-failed",
            "-Wno-unused-function", "-Wno-unused-variable", "-I", os.path.join(nat, "fake_hip"),
            "-I", os.path.join(tree, "include")]


def compile_units(tree, names, objdir):
    """-> error text or None; the named units of `tree` into objdir, all at once"""
    nat = os.path.join(tree, "tests", "native")
    procs = [(name, subprocess.Popen([clang(), "-x", "c++", "-c"] + flags(tree) + more +
                                     ["-o", os.path.join(objdir, name + ".o"), os.path.join(nat, src)],
                                     stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
             for name, src, more in units() if name in names]
    errs = [name + ": " + err[-1500:] for name, p in procs for err in [p.communicate()[1]] if p.returncode]
    return "\n".join(errs) or None


def link(objdirs, out):
    """objdirs: later directories win (the mutant's objects over the baseline's)"""
    objs = {}
    for d in objdirs:
        for name, _, _ in units():
            if os.path.exists(os.path.join(d, name + ".o")):
                objs[name] = os.path.join(d, name + ".o")
    r = subprocess.run([clang(), "-shared", "-Wl,-Bsymbolic", "-o", out] + [objs[n] for n, _, _ in units()],
                       capture_output=True, text=True)
    return r.stderr[-1500:] if r.returncode else None


def readers(tree):
    """unit -> the repository files it reads (clang++ -MM), relative to the tree"""
    nat = os.path.join(tree, "tests", "native")
    out = {}
    for name, src, more in units():
        r = subprocess.run([clang(), "-x", "c++", "-MM"] + flags(tree) + more + [os.path.join(nat, src)],
                           capture_output=True, text=True)
        if r.returncode:
            sys.exit("the unmutated tree does not compile: " + r.stderr[-1500:])
        deps = r.stdout.replace("\\\n", " ").split(":", 1)[1].split()
        out[name] = {os.path.relpath(os.path.realpath(d), os.path.realpath(tree)) for d in deps}
    return out


def copy_tree(src, dst):
    def ignore(d, names):
        return [n for n in names if n in SKIP_DIRS or n.endswith(SKIP_EXT)]
    shutil.copytree(src, dst, ignore=ignore, symlinks=True)
    with open(os.path.join(dst, "tests", "conftest.py"), "a") as f:
        f.write(FIXTURE)


def run_mutant(m, tree, base_objs, deps, stop_at_first, timeout):
    t0 = time.time()
    res = dict(id=m["id"], what=m["what"], failed=[], note="")
    with tempfile.TemporaryDirectory(prefix="mutant%02d_" % m["id"]) as tmp:
        work = os.path.join(tmp, "tree")
        copy_tree(tree, work)
        path = os.path.join(work, m["file"])
        text = open(path).read()
        if text.count(m["find"]) != m["count"]:
            res["outcome"] = "refused"
            res["note"] = "text found %d times, %d expected" % (text.count(m["find"]), m["count"])
            return res
        open(path, "w").write(text.replace(m["find"], m["replace"]))
        touched = {u for u, files in deps.items() if m["file"] in files}
        if not touched:
            res["outcome"], res["note"] = "refused", "no emulation unit reads " + m["file"]
            return res
        objs = os.path.join(tmp, "obj")
        os.mkdir(objs)
        err = compile_units(work, touched, objs)
        lib = os.path.join(tmp, "libkernels_on_cpu.so")
        err = err or link([base_objs, objs], lib)
        if err:
            res["outcome"], res["note"] = "killed", "does not build: " + err.strip().splitlines()[-1]
            return res
        env = dict(os.environ, RGB_AUDIT_EMU_SO=lib, PYTHONDONTWRITEBYTECODE="1")
        cmd = [sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-k", DESELECT, "-p", "no:cacheprovider",
               "-rfE", "--tb=no"] + (["-x"] if stop_at_first else []) + m["tests"]
        try:
            r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True, timeout=timeout)
            res["failed"] = re.findall(r"^(?:FAILED|ERROR) (\S+)", r.stdout, re.M)
            if r.returncode == 0:
                res["outcome"] = "survived"
            elif r.returncode == 1 and res["failed"]:
                res["outcome"] = "killed"
            elif r.returncode < 0 or r.returncode > 5:
                res["outcome"], res["note"] = "killed", "the test process died, status %d" % r.returncode
            else:
                res["outcome"], res["note"] = "error", (r.stdout + r.stderr)[-800:]
        except subprocess.TimeoutExpired:
            res["outcome"], res["note"] = "killed", "no end within %d s" % timeout
    res["seconds"] = round(time.time() - t0, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--list", default=os.path.join(HERE, "mutation_audit.json"))
    ap.add_argument("--only", default="")
    ap.add_argument("--jobs", type=int, default=max(1, min(4, (os.cpu_count() or 2) // 2)))
    ap.add_argument("--stop-at-first", action="store_true", help="pytest -x: one failing id per killed mutant")
    ap.add_argument("--subst", action="append", default=[])
    ap.add_argument("--timeout", type=int, default=300, help="seconds for the tests of one mutant (one that loops is killed)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    mutants = json.load(open(a.list))
    assert len({m["id"] for m in mutants}) == len(mutants), "mutant ids repeat"
    n_equiv = sum(1 for m in mutants if m.get("equivalent"))
    if 4 * n_equiv > len(mutants):
        sys.exit("%d of %d mutants are closed as equivalent: more than a quarter" % (n_equiv, len(mutants)))
    for s in a.subst:
        old, new = s.split("=", 1)
        for m in mutants:
            m["find"], m["replace"] = m["find"].replace(old, new), m["replace"].replace(old, new)
    if a.only:
        want = {int(x) for x in a.only.split(",")}
        mutants = [m for m in mutants if m["id"] in want]
    results = []
    with tempfile.TemporaryDirectory(prefix="mutation_audit_base_") as base:
        t0 = time.time()
        deps = readers(tree)
        err = compile_units(tree, {n for n, _, _ in units()}, base) or link([base], os.path.join(base, "base.so"))
        if err:
            sys.exit("the unmutated tree does not build: " + err)
        print("unmutated tree built in %.0f s; %d mutants, %d at a time" % (time.time() - t0, len(mutants), a.jobs), flush=True)
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            futs = [pool.submit(run_mutant, m, tree, base, deps, a.stop_at_first, a.timeout) for m in mutants]
            for m, f in zip(mutants, futs):
                r = f.result()
                r["equivalent"], r["gpu_only"], r["open"] = m.get("equivalent", ""), m.get("gpu_only", []), m.get("open", "")
                results.append(r)
                line = "%3d  %-9s %s" % (r["id"], r["outcome"], r["what"])
                if r["outcome"] == "killed":
                    line += "\n       " + ("%d tests: " % len(r["failed"]) + " ".join(r["failed"][:4]) +
                                           (" ..." if len(r["failed"]) > 4 else "") if r["failed"] else r["note"])
                elif r["outcome"] == "survived" and r["equivalent"]:
                    line += "\n       equivalent: " + r["equivalent"]
                elif r["outcome"] == "survived" and r["gpu_only"]:
                    line += "\n       killed on the GPU only: " + " ".join(r["gpu_only"])
                elif r["outcome"] == "survived" and r["open"]:
                    line += "\n       OPEN: " + r["open"]
                elif r["note"]:
                    line += "\n       " + r["note"]
                print(line, flush=True)
    if a.json:
        json.dump(results, open(a.json, "w"), indent=1)
    killed = [r for r in results if r["outcome"] == "killed"]
    surv = [r for r in results if r["outcome"] == "survived"]
    unexplained = [r["id"] for r in surv if not r["equivalent"] and not r["gpu_only"] and not r["open"]]
    stale = [r["id"] for r in killed if r["equivalent"] or r["open"]]
    broken = [r["id"] for r in results if r["outcome"] in ("refused", "error")]
    print("%d killed, %d survived (%d equivalent, %d killed on the GPU only, %d open, %d unexplained), %d refused or in error"
          % (len(killed), len(surv), sum(1 for r in surv if r["equivalent"]),
             sum(1 for r in surv if r["gpu_only"] and not r["equivalent"]),
             sum(1 for r in surv if r["open"] and not r["equivalent"] and not r["gpu_only"]), len(unexplained), len(broken)))
    if stale:
        print("closed as equivalent or open, but killed:", stale)
    if unexplained:
        print("unexplained survivors:", unexplained)
    return 1 if unexplained or broken or stale else 0


if __name__ == "__main__":
    sys.exit(main())
