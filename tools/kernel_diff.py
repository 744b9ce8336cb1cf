"""Compare the gfx950 machine code of two builds, kernel by kernel.

    python tools/kernel_diff.py LIB_OR_CODE_A LIB_OR_CODE_B

Each argument is a HIP shared library (*.so: its gfx950 code object is taken out of the fat binary), a code object (*.co / *.hsaco) or
an entry of radiosaber_amd's disk cache of run-time compiled kernels (*.rsco).  Both are disassembled (tools/lint_exec_restore.py) and
compared as text per kernel symbol, addresses and encodings stripped and local labels renumbered in order of appearance.  Prints the
kernel and instruction counts of both sides and the names that exist on one side only or whose instruction stream differs; two cache
entries also have their key texts compared (the device-source hash line apart).  Exit 0 when the kernel sets are equal and no stream
differs, else 1.  What a refactor of the device sources runs before anything goes near a GPU.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lint_exec_restore import code_of_cache_file, code_of_library, disassemble  # noqa: E402

SYMBOL = re.compile(r"^[0-9a-f]+ <([\w.$]+)>:$")
LOCAL = re.compile(r"^L\d+$")


def load(path):
    """-> (key text or None, code object bytes)"""
    if path.endswith(".rsco"):
        return code_of_cache_file(path)
    if path.endswith(".so"):
        return None, code_of_library(path)
    return None, open(path, "rb").read()


def kernels(code):
    """code object -> {symbol: [instruction text, ...]}"""
    out, cur, labels = {}, None, {}
    for raw in disassemble(code).split("\n"):
        line = raw.strip()
        m = SYMBOL.match(line)
        if m:
            name = m.group(1)
            if LOCAL.match(name):
                cur.append(labels.setdefault(name, "L#%d" % len(labels)) + ":")
            else:
                cur, labels = out.setdefault(name, []), {}
            continue
        if cur is None or not line or line == "..." or line.startswith("Disassembly") or "file format" in line:  # ("...": padding behind the last kernel)
            continue
        ins = line.split("//")[0].rstrip()  # (the comment holds the address and the encoding)
        ins = re.sub(r"\bL\d+\b", lambda t: labels.setdefault(t.group(0), "L#%d" % len(labels)), ins)
        if ins:
            cur.append(ins)
    return out


def count(ks):
    return sum(1 for k in ks.values() for i in k if not i.endswith(":"))


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    (key_a, code_a), (key_b, code_b) = load(argv[0]), load(argv[1])
    a, b = kernels(code_a), kernels(code_b)
    print(f"A {argv[0]}: {len(a)} kernels, {count(a)} instructions")
    print(f"B {argv[1]}: {len(b)} kernels, {count(b)} instructions")
    bad = 0
    for name in sorted(set(a) - set(b)):
        bad += 1
        print(f"only in A: {name}")
    for name in sorted(set(b) - set(a)):
        bad += 1
        print(f"only in B: {name}")
    for name in sorted(set(a) & set(b)):
        if a[name] != b[name]:
            bad += 1
            first = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
            print(f"differs: {name} ({len(a[name])} against {len(b[name])} lines, first at line {first})")
    if key_a is not None and key_b is not None:
        strip = lambda k: [l for l in k.split("\n") if not l.startswith("src ")]
        if strip(key_a) != strip(key_b):
            bad += 1
            print("cache key texts differ beyond the device-source hash")
        else:
            print("cache key texts equal apart from the device-source hash" if key_a != key_b else "cache key texts equal")
    print("identical" if not bad else f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
