"""Identity of the Python binding's computed tables with the hand-written ones of another commit (CPU, no library).

    python tools/binding_identity.py [REV]          (default HEAD~1; DESIGN.md section 33, profiles/binding_refactor.txt)

``phyloformer_amd/engine.py`` and ``hostio.py`` of REV are read from git and executed as modules beside this tree's
package.  Compared: ``SIGNATURES`` name by name, return type by return type and argument by argument - a scalar must be
the identical ctypes type, a pointer may differ between ``POINTER(x)`` and ``c_void_p`` only, and every such position is
listed; ``CALL_TIME_SYMBOLS``; the constants the header now supplies; ``dir(Engine)``.  Exit status 1 on any other
difference."""
import ctypes as C
import os
import subprocess
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
CONSTANTS = {"engine": ("ABI_VERSION", "UNIQUE_ID_BYTES", "PF_OK", "PF_EINVAL", "PF_EHIP", "PF_ERCCL", "PF_ENOMEM", "PF_ESTATE"),
             "hostio": ("PF_EIO", "PF_FASTA_EBYTE", "PF_FASTA_ERAGGED", "PF_FASTA_ENOHEADER", "PF_FASTA_EEMPTY", "PF_FASTA_ECAP",
                        "PF_FASTA_EUTF8")}


def module_at(rev, name):
    """``phyloformer_amd/<name>.py`` of ``rev`` as a module of this tree's package."""
    path = f"phyloformer_amd/{name}.py"
    src = subprocess.run(["git", "show", f"{rev}:{path}"], capture_output=True, text=True, cwd=REPO, check=True).stdout
    mod = types.ModuleType(f"phyloformer_amd._{name}_at_rev")
    mod.__package__, mod.__file__ = "phyloformer_amd", os.path.join(REPO, path)
    sys.modules[mod.__name__] = mod
    exec(compile(src, f"{rev}:{path}", "exec"), mod.__dict__)
    return mod


def kind(t):
    return "void" if t is None else t.__name__


def main(argv):
    rev = argv[0] if argv else "HEAD~1"
    from phyloformer_amd import engine, hostio
    old = {"engine": module_at(rev, "engine"), "hostio": module_at(rev, "hostio")}
    new = {"engine": engine, "hostio": hostio}
    bad, pointers = [], []
    was, now = old["engine"].SIGNATURES, engine.SIGNATURES
    if set(was) != set(now):
        bad.append(f"names: only in {rev} {sorted(set(was) - set(now))}, only here {sorted(set(now) - set(was))}")
    for name in sorted(set(was) & set(now)):
        (r0, a0), (r1, a1) = was[name], now[name]
        if r0 is not r1:
            bad.append(f"{name}: returns {kind(r0)}, here {kind(r1)}")
        if len(a0) != len(a1):
            bad.append(f"{name}: {len(a0)} arguments, here {len(a1)}")
            continue
        for i, (x, y) in enumerate(zip(a0, a1)):
            if x is y:
                continue
            if y is C.c_void_p and issubclass(x, C._Pointer):
                pointers.append(f"{name}[{i}] {x.__name__}")
            else:
                bad.append(f"{name}[{i}]: {kind(x)}, here {kind(y)}")
    print(f"SIGNATURES: {len(now)} names, {sum(len(a) for _, a in now.values())} arguments; besides the positions below every "
          "return type and argument is the identical ctypes type")
    print(f"POINTER(x) in {rev}, c_void_p here: {len(pointers)} positions")
    for p in pointers:
        print("  " + p)
    ct0, ct1 = old["engine"].CALL_TIME_SYMBOLS, engine.CALL_TIME_SYMBOLS
    print(f"CALL_TIME_SYMBOLS: {len(ct0)} in {rev}, {len(ct1)} here; added {sorted(ct1 - ct0)}; removed {sorted(ct0 - ct1)}")
    for where, names in CONSTANTS.items():
        pairs = [(n, getattr(old[where], n), getattr(new[where], n)) for n in names]
        bad += [f"{where}.{n}: {a}, here {b}" for n, a, b in pairs if a != b or type(a) is not type(b)]
        print(f"{where}: " + " ".join(f"{n}={b}" for n, _, b in pairs))
    d0, d1 = set(dir(old["engine"].Engine)), set(dir(engine.Engine))
    if d0 != d1:
        bad.append(f"dir(Engine): only in {rev} {sorted(d0 - d1)}, only here {sorted(d1 - d0)}")
    print(f"dir(Engine): {len(d1)} names here, {len(d0)} in {rev}")
    print("\n".join("DIFFERENT " + b for b in bad) if bad else "no other difference")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
