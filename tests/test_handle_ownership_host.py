"""Ownership of a handle's device memory and events, read off the sources -- no device, no library.  csrc/bogp_handle.h defines the three
owning types (DevBuf, MappedBuf, EventPool); every allocation, pinned block and event of the host layer goes through them, so the HIP calls
that create or release one occur nowhere else in the host layer, and the handle keeps no capacity field beside a pointer."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "bayesian-optimization_amd", "csrc")
DEFINING = os.path.join(CSRC, "bogp_handle.h")
# the six calls (hipEventCreate covers hipEventCreateWithFlags), as calls: error messages may still name them
CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipEventCreate\w*|hipEventDestroy)\s*\(")


def _code(path):
    """The file without its comments (string literals stay: CALLS wants an opening parenthesis behind the name)."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def test_allocation_and_event_calls_live_in_the_defining_header_only():
    host = sorted(glob.glob(os.path.join(CSRC, "bogp_*.hip")))
    headers = sorted(set(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc")) + glob.glob(os.path.join(ROOT, "include", "*.h"))))
    assert len(host) >= 12 and DEFINING in headers
    found = {}
    for path in host + [p for p in headers if p != DEFINING]:
        hits = sorted(set(CALLS.findall(_code(path))))
        if hits:
            found[os.path.relpath(path, ROOT)] = hits
    assert not found, found
    # ... and the defining header does hold all six: the search above looks for the right names
    assert set(CALLS.findall(_code(DEFINING))) == {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreateWithFlags", "hipEventDestroy"}


def test_the_handle_keeps_no_capacity_field():
    src = _code(DEFINING)
    start = src.index("struct bogp_handle {")
    body = src[start : src.index("\n};", start)]
    assert "DevBuf<double> dX" in body and "SpanTimer timer;" in body and "MappedBuf hfit;" in body  # the struct, not a forward declaration
    caps = set(re.findall(r"\b(\w*_cap\w*|cap_\w+)\b", body))
    assert caps == {"cap_ld", "cap_d", "cap_nt"}, sorted(caps)  # the training set's geometry, not buffer capacities
