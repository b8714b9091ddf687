"""CPU: include/goldsrl_swarmrules.h (feedback rules on the Swarm env, whole episodes in one launch) -- the two functions it
declares are exported by libgoldsrl.so and bound in goldsrl/_ffi_swarmrules.py, the signature dict names exactly the declared set
and shares nothing with the pinned goldsrl.h, and a null handle is refused without a device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_swarmrules
    declared = _declared("goldsrl_swarmrules.h")
    assert declared == {"grl_swarm_rules", "grl_swarm_rules_read"}
    assert set(_ffi_swarmrules.SWARMRULES_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    lib = _ffi.load_library(extra_signatures=_ffi_swarmrules.SWARMRULES_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_swarmrules.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_swarmrules.h")
    assert callable(_ffi_swarmrules.swarm_rules)


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_swarmrules
    lib = _ffi.load_library(extra_signatures=_ffi_swarmrules.SWARMRULES_SIGNATURES)
    assert lib.grl_swarm_rules(None, None, None, 1, 1, 0, -1) == _ffi.E_INVALID
    assert lib.grl_swarm_rules_read(None, b"rewards", None, 0) == _ffi.E_INVALID
