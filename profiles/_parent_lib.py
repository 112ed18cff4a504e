"""What the bench scripts with a --parent-lib option share: a measuring step as a child process of its own, through
the in-tree libmuz.so or through another build (MUZ_LIB), and the parent-then-new run that fills a log."""
import os
import subprocess
import sys


def parent_lib(argv):
    """the path after --parent-lib, or None"""
    return argv[argv.index("--parent-lib") + 1] if "--parent-lib" in argv else None


def run_child(script, args, lib=None, limit=300):
    """`script args...` in a process of its own under a time limit, through library `lib` (None: the in-tree one)"""
    env = {**os.environ, **({"MUZ_LIB": os.path.abspath(lib)} if lib else {})}
    return subprocess.run([sys.executable, os.path.abspath(script), *args], capture_output=True, text=True,
                          timeout=limit, env=env)


def main(script, log, argv):
    """The script's --child step, first through --parent-lib's library when one is given, then through the in-tree
    one; both outputs, headed by which library ran, go to stdout and to `log`."""
    parent = parent_lib(argv)
    out = []
    for lib in ([parent] if parent else []) + [None]:
        r = run_child(script, ["--child"], lib)
        head = ("[parent commit's library]\n" if lib else "[this commit]\n") if parent else ""
        out.append(head + r.stdout)
        sys.stdout.write(out[-1])
        sys.stderr.write(r.stderr)
        sys.stdout.flush()
        if r.returncode != 0:
            return r.returncode
    with open(log, "w") as f:
        f.write("".join(out))
    return 0
