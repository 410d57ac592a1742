#!/usr/bin/env python
"""DESIGN 4.11, per kernel: do two trees generate the same device code for the decode and teacher kernels? (no GPU needed)

    python tools/asm_identity.py emit OUT_DIR [TREE]      # TREE: a checkout of this repository (default: this one)
    python tools/asm_identity.py compare DIR_A DIR_B      # one line per file; exit status 1 if any file differs
    ... --files a.hip b.hip                               # either command: these files of csrc/ (default: FILES)

``emit`` compiles each file device-only to assembly with ``build.COMPILE_FLAGS`` and the include path of
``build._compile``. ``compare`` splits each assembly text by kernel symbol (every ``.amdhsa_kernel NAME``), takes a
kernel's text from its label ``NAME:`` to the ``.end_amdhsa_kernel`` of its descriptor (the ``.amdhsa_*`` resource lines
included) and asks that both sides define the same symbols with byte-identical text. The order of the kernels in the file
and the ``__hip_cuid_<hash>`` symbol (outside every kernel's text) are the only differences it lets pass. The assembler's
local labels carry the kernel's position in the file (``.LBB<k>_<n>``, k from the ``.Lfunc_end<k>`` behind the kernel), so
where the order moves that ordinal moves with it: each kernel's own ordinal is written as ``#`` before the comparison and
the blanks that align the comment behind such a label (their number follows k's digits) as one, and nothing else is. It is a text comparison keyed by symbol: it reads no instruction."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rl4co_amd import build as B  # noqa: E402

FILES = ["am_decode.hip", "am_decode_ms.hip", "am_decode_ms_f16.hip", "am_decode_beam.hip", "am_teacher.hip",
         "am_teacher_mma.hip", "am_teacher_mma_f16.hip"]


def emit(out: Path, tree: Path, files=FILES) -> None:
    out.mkdir(parents=True, exist_ok=True)
    procs = [(name, subprocess.Popen(
        [B._hipcc(), *B.COMPILE_FLAGS, f"-I{tree / 'include'}", "--cuda-device-only", "-S",
         str(tree / "rl4co_amd" / "csrc" / name), "-o", str(out / (name + ".s"))], stderr=subprocess.PIPE, text=True))
        for name in files]
    for name, p in procs:
        err = p.communicate()[1]
        if p.returncode != 0:
            raise SystemExit(f"hipcc failed on {name}:\n{err}")


def kernels(text: str) -> dict:
    """{kernel symbol: its text from the label to the end of its descriptor}"""
    lines = text.splitlines(keepends=True)
    label = {ln.split(":")[0]: i for i, ln in enumerate(lines) if ln[:1] not in "\t .;\n" and ":" in ln}
    out = {}
    for i, ln in enumerate(lines):
        if ln.strip().startswith(".amdhsa_kernel "):
            name = ln.split()[1]
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            k = next(m.group(1) for m in (re.match(r"\.Lfunc_end(\d+):", x) for x in lines[end:]) if m)  # its position in the file
            text = "".join(lines[label[name]:end + 1]).replace("BB%s_" % k, "BB#_")
            out[name] = re.sub(r"^(\.LBB#_\d+:) +;", r"\1 ;", text, flags=re.M)  # the comment column moves with k's digits
    return out


def compare(a: Path, b: Path, files=FILES) -> int:
    bad = 0
    for name in files:
        ka, kb = kernels((a / (name + ".s")).read_text()), kernels((b / (name + ".s")).read_text())
        only = sorted(set(ka) ^ set(kb))
        differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        same_order = list(ka) == list(kb)
        ok = not only and not differ
        bad += not ok
        print(f"{name}: {len(ka)} kernels / {len(kb)} kernels, {len(only)} on one side only, {len(differ)} with different "
              f"text, order {'kept' if same_order else 'moved'}: {'IDENTICAL' if ok else 'DIFFERENT'}")
        for k in (only + differ)[:8]:
            print(f"    {'one side only' if k in only else 'text differs'}: {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    argv, files = sys.argv[1:], FILES
    if "--files" in argv:
        argv, files = argv[:argv.index("--files")], argv[argv.index("--files") + 1:]
    if not files:
        raise SystemExit(__doc__)
    if len(argv) in (2, 3) and argv[0] == "emit":
        emit(Path(argv[1]), Path(argv[2]).resolve() if len(argv) > 2 else ROOT, files)
    elif len(argv) == 3 and argv[0] == "compare":
        sys.exit(compare(Path(argv[1]), Path(argv[2]), files))
    else:
        raise SystemExit(__doc__)
