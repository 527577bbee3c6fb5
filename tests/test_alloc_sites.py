"""Source lint (no GPU): every device allocation that can run after tsp_create goes through alloc_group(), whose
failure leaves a group of buffers null with capacity 0, or -- per-call scratch -- through scratch_alloc() (TSP_SCRATCH_ALLOC), and
every allocation site has a name of its own that the GPU tests (test_gpu_alloc_failure.py, test_gpu_scratch_alloc_failure.py,
test_gpu_upload_alloc_failure.py) make fail."""
import glob
import os
import re

from test_gpu_alloc_failure import GENERIC_SITES, POSTPASS_SITES, RENDER_SITES
from test_gpu_scratch_alloc_failure import SCRATCH_SITES
from test_gpu_upload_alloc_failure import UPLOAD_SITES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "topsy_amd", "csrc")
# functions that may call hipMalloc themselves: the two helpers and context creation
RAW_ALLOWED = {"alloc_group", "scratch_alloc", "create_resources"}
FUNC_DEF = re.compile(r"^(?!return\b|else\b|if\b|for\b|while\b|switch\b)[A-Za-z_][\w:<>,\s\*&]*?\b(\w+)\s*\([^;]*$")
SITE = re.compile(r'\{\s*"(\w+)"\s*,\s*(?:\(void\s*\*\*\)\s*)?&|\bSITE\("(\w+)"\)')


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert any(f.endswith(".hip") for f in files) and any(f.endswith(".h") for f in files), CSRC
    for path in files:
        with open(path) as f:
            yield os.path.basename(path), f.read()


def enclosing_functions(text):
    """(line number, name of the function defined last above it at column 0) for every raw hipMalloc call"""
    current = None
    for no, line in enumerate(text.splitlines(), 1):
        if not line.startswith((" ", "\t", "#", "/", "}", "{")):
            m = FUNC_DEF.match(line)
            if m:
                current = m.group(1)
        if re.search(r"\bhipMalloc\s*\(", line.split("//")[0]):
            yield no, current


def test_raw_hipmalloc_only_in_the_helper_and_creation():
    bad = [f"{name}:{no} in {fn}" for name, text in sources() for no, fn in enclosing_functions(text) if fn not in RAW_ALLOWED]
    assert not bad, "device allocations outside alloc_group(), scratch_alloc() and context creation: " + ", ".join(bad)


def test_the_lint_sees_the_helper():
    found = {fn for _, text in sources() for _, fn in enclosing_functions(text)}
    assert "alloc_group" in found and "scratch_alloc" in found and "create_resources" in found, found


def test_scratch_buffers_are_allocated_by_the_helper_only():
    """a DeviceScratch has no alloc() of its own: no line of the sources calls one (comments aside)"""
    bad = [f"{name}:{no}" for name, text in sources() for no, line in enumerate(text.splitlines(), 1)
           if re.search(r"(\.|->)\s*alloc\s*\(", line.split("//")[0])]
    assert not bad, "scratch allocated without scratch_alloc() / TSP_SCRATCH_ALLOC: " + ", ".join(bad)
    macro = [f"{name}:{no}" for name, text in sources() for no, line in enumerate(text.splitlines(), 1)
             if "TSP_SCRATCH_ALLOC(" in line.split("//")[0] and not line.lstrip().startswith("#define")
             and not re.search(r'TSP_SCRATCH_ALLOC\(ctx, (SITE\("\w+"\)|\w+_site\[\w+\]), ', line)]
    assert not macro, "TSP_SCRATCH_ALLOC without a SITE(\"name\") (or an entry of a table of them): " + ", ".join(macro)


def test_site_names_are_unique_and_covered():
    names = [a or b for _, text in sources() for a, b in SITE.findall(re.sub(r"//[^\n]*", "", text))]      # (comments aside)
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, f"allocation sites sharing a name: {dup}"
    covered = set().union(*RENDER_SITES.values(), GENERIC_SITES, POSTPASS_SITES, *SCRATCH_SITES.values(), *UPLOAD_SITES.values())
    assert set(names) == covered, (f"sites no GPU test makes fail: {sorted(set(names) - covered)}; "
                                   f"sites the tests expect that the sources lack: {sorted(covered - set(names))}")
