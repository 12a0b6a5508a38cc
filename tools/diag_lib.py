"""Gate of the tools whose knob only the diagnostic library reads (`make -C bayesianneuralnetworks_amd/csrc diag`, loaded through
BNN_HIP_LIB): `require(what)` ends the process with one line, before any GPU work, unless the loaded library says it is one --
a fresh diagnostic library's bnn_last_error() is its build note.   usage (shell): python tools/diag_lib.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NOTE = b"diagnostic build (BNN_DIAG)"


def require(what):
    from bayesianneuralnetworks_amd import _lib
    if _lib.load().bnn_last_error() != NOTE:
        sys.exit("%s needs the diagnostic library: make -C bayesianneuralnetworks_amd/csrc diag, then "
                 "BNN_HIP_LIB=<repo>/bayesianneuralnetworks_amd/libbnn_hip_diag.so (loaded: %s)" % (what, _lib.LIB_PATH))


if __name__ == "__main__":
    require("this step")
