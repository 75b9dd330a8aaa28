"""Per-kernel comparison of the gfx950 code objects of two compiled .o files (hipcc fat objects): for every kernel symbol, are the metadata
notes (registers, scratch, LDS, spill counts, kernarg layout) equal, and is the disassembly equal?  For a change that must leave device code alone.
One thing is masked in the disassembly: the 32-bit literals of the s_add_u32 / s_addc_u32 pair that follows an s_getpc_b64 -- a pc-relative
address of a table or function, which moves when the order of the kernels in the object does (with --strict nothing is masked).
Addresses, encodings and the disassembler's comments are not compared; instructions, registers, immediates and relative branch offsets are.
usage: python tools/code_object_diff.py [--strict] old/build/bc7.o new/build/bc7.o        exit status 0 = all equal"""
import re, subprocess, sys, tempfile
from kernel_resources import LLVM, unbundle, kernel_notes, note_field

GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):(\d+)\]$")


def notes_by_kernel(co):
    return {note_field(b, "name"): b for b in kernel_notes(co)}


def disassembly_by_symbol(co, strict):
    """symbol -> its instructions, one string each, without addresses and encodings"""
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    out, cur, pc = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), []); pc = None
            continue
        if cur is None or not line.startswith("\t"): continue
        ins = re.sub(r"\s+", " ", line.split("//")[0]).strip()
        if not ins: continue
        g = GETPC.match(ins)
        if g: pc = (g.group(1), g.group(2), 0)                    # the register pair, instructions seen since
        elif pc and not strict:
            lo, hi, age = pc
            ins, k = re.subn(rf"^(s_add_u32 s{lo}, s{lo}, |s_addc_u32 s{hi}, s{hi}, )\S+$", r"\1<pc-relative>", ins)
            pc = None if (ins.startswith("s_addc_u32") and k) or age >= 4 else (lo, hi, age + 1)
        cur.append(ins)
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--strict"]
    strict = "--strict" in sys.argv[1:]
    if len(args) != 2: sys.exit(__doc__)
    sides = []
    for obj in args:
        with tempfile.TemporaryDirectory() as d:
            co = unbundle(obj, d)
            sides.append((notes_by_kernel(co), disassembly_by_symbol(co, strict), open(co, "rb").read()))
    (na, da, ba), (nb, db, bb) = sides
    only_a, only_b = sorted(set(na) - set(nb)), sorted(set(nb) - set(na))
    for name in only_a: print(f"only in {args[0]}: {name}")
    for name in only_b: print(f"only in {args[1]}: {name}")
    bad_notes = bad_code = lines = 0
    for name in sorted(set(na) & set(nb)):
        notes_equal = na[name] == nb[name]
        a, b = da.get(name), db.get(name)
        code_equal = a is not None and a == b
        lines += len(a or [])
        bad_notes += not notes_equal; bad_code += not code_equal
        if not (notes_equal and code_equal):
            where = "" if code_equal or a is None or b is None else f" (first difference at instruction {next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))}; {len(a)} / {len(b)} instructions)"
            print(f"{name}: notes {'equal' if notes_equal else 'DIFFER'}, disassembly {'equal' if code_equal else 'DIFFERS'}{where}")
    # device functions that are not kernels (no notes of their own) count towards the disassembly as well
    others = sorted((set(da) | set(db)) - set(na) - set(nb))
    bad_other = sum(1 for s in others if da.get(s) != db.get(s))
    for s in others:
        if da.get(s) != db.get(s): print(f"{s} (not a kernel): disassembly DIFFERS")
    same = not (only_a or only_b or bad_notes or bad_code or bad_other)
    print(f"{len(set(na) & set(nb))} kernels in both ({len(only_a)} / {len(only_b)} in one only): notes differ in {bad_notes}, disassembly differs in {bad_code} "
          f"({lines} instructions compared, {'nothing masked' if strict else 'pc-relative literals masked'}); {len(others)} other symbols, {bad_other} differ; "
          f"code objects {'byte-identical' if ba == bb else 'not byte-identical'}: {'EQUAL' if same else 'DIFFERENT'}")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
