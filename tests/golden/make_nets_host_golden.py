"""Writes tests/golden/nets_host.json: what the initialisers and packers of nets.py, stochastic.py and muzero_dog.py
build on the host, as names and hashes (tests/_nets_host.py), recorded from a given copy of the package.

    python tests/golden/make_nets_host_golden.py PKG_DIR

PKG_DIR holds the package of the commit before the one-construction-path refactor (``git archive`` of
exploring-muzero-on-dog_amd/, with libmuz.so beside it); tests/test_nets_host.py holds the current package to it.
No GPU: the packers are built at device="cpu" with the FiLM-table kernel (prepare) left out, and the spec is taken
where the weight table would be filled from it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "nets_host.json")


def main(pkg_dir):
    sys.path.insert(0, ROOT)
    import muzpkg
    muzpkg.PKG_DIR = os.path.abspath(pkg_dir)
    muzpkg.load()
    from exploring_muzero_on_dog_amd import nets as N
    from tests import _nets_host as H

    inits = H.initialisers()
    rec = {"init": {game: H.init_record(fn) for game, fn in inits.items()}, "pack": {}}
    specs = []
    N._Packer._fill = staticmethod(lambda struct, spec, base: specs.append(spec))
    for game, cls in H.packers().items():
        cls.prepare = lambda self: None
        C, A = H.SHAPES[game]
        args = {"det": (C, A), "classic": (C,), "dog": ()}[game]
        net = cls(H.pack_params(inits[game]), *args, device="cpu")
        rec["pack"][game] = H.pack_record(net._chunks, specs[-1])
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main(sys.argv[1])
