"""Host-side checks of the MXFP4 GEMM interface (no GPU): the ABI version, the two new entry points in the binding and in the
public header, and the argument check of ``LlamaEngine.use_fp4`` that must not reach the library."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["emu_linear_fp4w_gemm_bf16", "emu_llama_release_bf16"]


def test_abi_version_is_6():
    from emu_amd import _lib
    assert _lib.ABI_VERSION == 6
    src = open(os.path.join(ROOT, "emu_amd", "csrc", "engine.hip")).read()
    assert re.search(r"int emu_version\(void\) \{ return 6; \}", src)


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_have_prototypes_and_declarations(name):
    from emu_amd import _lib
    protos = next(v for v in vars(_lib).values() if isinstance(v, dict) and "emu_version" in v)
    assert name in protos
    header = open(os.path.join(ROOT, "include", "emu_hip.h")).read()
    assert re.search(r"^int " + name + r"\(", header, re.M)
    # the GEMM takes the thin stream's argument list
    if name == "emu_linear_fp4w_gemm_bf16":
        assert protos[name] == protos["emu_linear_fp4w_thin_bf16"]


def test_all_rows_without_wide_is_a_value_error_before_the_library():
    from emu_amd.llama import LlamaEngine

    class NoLibrary:
        """Stands for an engine: any attribute the method would need to reach the library (handle, ctx, the quantiser) is an error."""
        def __getattr__(self, name):
            raise AssertionError(f"use_fp4 touched {name!r} before refusing its arguments")
    with pytest.raises(ValueError, match="all_rows"):
        LlamaEngine.use_fp4(NoLibrary(), True, all_rows=True, wide=False)
    with pytest.raises(ValueError, match="all_rows"):
        LlamaEngine.use_fp4(NoLibrary(), True, all_rows=True)
