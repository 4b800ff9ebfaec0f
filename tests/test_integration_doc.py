"""INTEGRATION.md section B is the reference-side binding of the drop-in boundary (what a maintainer of lh3/psmc would
paste into em.c).  Prose rots: these tests extract the C blocks as written and check every psmc_hip_* entry point they
call against our public header and the symbols libpsmc_hip.so exports -- a renamed or dropped entry point, or a
fragment whose argument count drifted from the declaration, fails here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_blocks(section_title):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text.split(section_title, 1)[1]
    sec = re.split(r"\n## ", sec, 1)[0]
    return re.findall(r"```c\n(.*?)```", sec, flags=re.S)


def test_section_b_snippet_names_exported_entry_points():
    blocks = c_blocks("## B. Keep the reference's host code")
    assert blocks and "hip_estep" in blocks[0]
    lib = os.path.join(ROOT, "psmc_amd")
    assert os.path.exists(os.path.join(lib, "libpsmc_hip.so")), "build the library first (__graft_entry__.build)"
    # every psmc_hip_* symbol the snippet calls is declared in the header and exported by the library
    used = set(re.findall(r"\b(psmc_hip_[a-z_]+)\s*\(", blocks[0]))
    assert used
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(lib, "libpsmc_hip.so")], capture_output=True, text=True).stdout
    header = open(os.path.join(ROOT, "include", "psmc_hip.h")).read()
    for s in used:
        assert re.search(r"\b%s\b" % s, nm), s
        assert re.search(r"\b%s\s*\(" % s, header), s


def test_section_b_and_d_fragments_name_real_entry_points():
    """The one-line fragments (decode calls, batch and group bindings) are not complete C; check that every entry point
    they name exists with the argument count shown."""
    header = open(os.path.join(ROOT, "include", "psmc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    frags = "".join(re.findall(r"```c\n(.*?)```", text, flags=re.S)[1:])
    frags = re.sub(r"/\*.*?\*/", "", frags, flags=re.S)
    for m in re.finditer(r"\b(psmc_hip_[a-z_]+)\s*\(([^;]*?)\);", frags, flags=re.S):
        name, args = m.group(1), m.group(2)
        decl = re.search(r"\b%s\s*\(([^;]*?)\);" % name, header, flags=re.S)
        assert decl, name
        assert len(args.split(",")) == len(decl.group(1).split(",")), (name, args, decl.group(1))
