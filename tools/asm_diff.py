"""Compare two device listings (make asm: build/<unit>.s per translation unit with kernels; concatenate
them, `cat build/context.s build/detect.s build/encode.s`) kernel by kernel.

    python tools/asm_diff.py OLD.s NEW.s

Per function of either listing one line: "identical" (same text), "same opcode counts" (the
instructions differ only in operands or order), or the opcodes whose counts differ (old -> new).
Lines naming __hip_cuid (a hash of the source path) and the function ordinal in block labels
(which moves when a header is reordered) are ignored. Build both listings at the same checkout
path. Exit status 0.
"""
import collections
import re
import sys


def functions(path):
    """name -> list of body lines (between the function's label and its .Lfunc_end)."""
    out, name, body = {}, None, []
    for line in open(path):
        if "__hip_cuid" in line:
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
        elif name and re.match(r"\.Lfunc_end\d+:", line):
            out[name], name = body, None
        elif name:  # block labels carry the function's ordinal in the file (.LBB<fn>_<block>)
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip()))
    return out


def opcodes(body):
    ops = collections.Counter()
    for line in body:
        tok = line.split()
        if tok and not tok[0].startswith(".") and not tok[0].endswith(":"):
            ops[tok[0]] += 1
    return ops


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    tally = collections.Counter()
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "only in " + ("new" if name in new else "old")
        elif old[name] == new[name]:
            verdict = "identical"
        else:
            a, b = opcodes(old[name]), opcodes(new[name])
            diff = [f"{op} {a[op]}->{b[op]}" for op in sorted(set(a) | set(b)) if a[op] != b[op]]
            verdict = ", ".join(diff) if diff else "same opcode counts"
        tally["identical" if verdict == "identical" else "same opcode counts" if verdict == "same opcode counts" else "differs"] += 1
        print(f"{name[:70]:70s} {verdict}")
    print("# " + ", ".join(f"{k}: {v}" for k, v in sorted(tally.items())))


if __name__ == "__main__":
    main()
