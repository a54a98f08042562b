"""The binding's prototypes come from include/phyloformer_amd.h (phyloformer_amd/cabi.py): the
parser on header texts written here, on the real header, the banner rule for functions a library may lack, and the
generated pass-through methods over the built library with a null handle.  No GPU."""
import ctypes as C
import os
import re
import types

import pytest

from phyloformer_amd import cabi, engine

# tests/test_host.py::test_abi_symbols_exported's own pattern
DECLARED = r"^(?:int64_t|uint64_t|int32_t|int|void|const char\*)\s+(pf_\w+)\("

SMALL = """
/* int pf_fake(int32_t a); is only talked about, and so is
 * int pf_fake2(void);
 */
#define PF_ABI_VERSION 7
#define PF_NEG (-16)
typedef enum pf_status {
    PF_OK = 0,
    PF_EBAD = -3,  /* int pf_fake3(void); */
    PF_ELAST = -4
} pf_status;
typedef struct pf_handle pf_handle_t;
// int pf_fake4(void);
int pf_three(pf_handle_t* h, const uint8_t* idx,   /* the input */
             int32_t B,
             float* out);
void pf_nothing(pf_handle_t* b);
const char* pf_text(void);
int pf_none();
/* ---- an addition (additive to ABI 7) ----
 *
 * int pf_fake5(void); */
uint64_t pf_late(int a, int32_t b, int64_t c, uint64_t d, size_t e, const char* f, char* g, const char* const* h,
                 pf_handle_t** i, const void* j, double* k, int32_t);
/* a comment that is no banner, and says (additive to ABI 7) */
int64_t pf_late2(void);
/* ---- back to the base ---- */
int32_t pf_base(void);
"""


def test_parser_on_a_small_header():
    protos, consts = cabi.parse(SMALL)
    assert list(protos) == ["pf_three", "pf_nothing", "pf_text", "pf_none", "pf_late", "pf_late2", "pf_base"]      # no pf_fake*
    assert consts == {"PF_ABI_VERSION": 7, "PF_NEG": -16, "PF_OK": 0, "PF_EBAD": -3, "PF_ELAST": -4}
    three = protos["pf_three"]                                                          # a prototype over three lines
    assert three.restype is C.c_int and three.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert three.text == "int pf_three(pf_handle_t* h, const uint8_t* idx, int32_t B, float* out);"
    assert protos["pf_nothing"].restype is None and protos["pf_nothing"].argtypes == [C.c_void_p]
    assert protos["pf_text"].restype is C.c_char_p and protos["pf_text"].argtypes == []          # (void)
    assert protos["pf_none"].argtypes == []
    late = protos["pf_late"]                                                            # every entry of the type table
    assert late.restype is C.c_uint64
    assert late.argtypes == [C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.c_char_p, C.c_char_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    assert protos["pf_late2"].restype is C.c_int64 and protos["pf_base"].restype is C.c_int32
    assert {n for n, p in protos.items() if p.call_time} == {"pf_late", "pf_late2"}


@pytest.mark.parametrize("proto", ["int pf_bad(unsigned int x);", "int pf_bad(float x);", "double pf_bad(void);",
                                   "int pf_bad(void x);", "int pf_bad(pf_handle_t h);", "int pf_bad(long long x);"])
def test_a_type_outside_the_table_raises_and_names_the_prototype(proto):
    with pytest.raises(TypeError, match=r"pf_bad\("):
        cabi.parse("int pf_good(void);\n" + proto + "\n")


@pytest.fixture(scope="module")
def header(repo):
    with open(os.path.join(repo, "include", "phyloformer_amd.h")) as fh:
        return fh.read()


def test_the_real_header(header):
    declared = re.findall(DECLARED, header, re.M)
    assert len(declared) == len(set(declared)) > 100 and set(declared) == set(cabi.PROTOTYPES) == set(engine.SIGNATURES)
    for name, p in cabi.PROTOTYPES.items():
        inside = p.text[p.text.index("(") + 1:p.text.rindex(")")]
        assert len(p.argtypes) == (0 if inside == "void" else inside.count(",") + 1), p.text
        assert engine.SIGNATURES[name] == (p.restype, p.argtypes)
    for name in ("PF_OK", "PF_EINVAL", "PF_EHIP", "PF_ERCCL", "PF_ENOMEM", "PF_ESTATE"):
        assert getattr(engine, name) == cabi.CONSTANTS[name] == int(re.search(rf"\b{name} = (-?\d+)", header).group(1))
    from phyloformer_amd import hostio
    for name in ("PF_FASTA_EBYTE", "PF_FASTA_ERAGGED", "PF_FASTA_ENOHEADER", "PF_FASTA_EEMPTY", "PF_FASTA_ECAP", "PF_FASTA_EUTF8"):
        assert getattr(hostio, name) == int(re.search(rf"#define {name} \((-\d+)\)", header).group(1))
    assert hostio.PF_EIO == -6 and engine.PF_ESTATE == -5 and hostio.PF_FASTA_EUTF8 == -21
    assert engine.SIGNATURES["pf_boot_counts"][1][2] is C.c_uint64 and engine.SIGNATURES["pf_debug_read"][1][3] is C.c_int64


def test_the_banner_says_which_functions_a_library_may_lack(header):
    marked, under = set(), False
    for line in header.split("\n"):
        if line.startswith("/* ----"):
            under = re.search(r"\(additive to ABI \d+\)", line) is not None
        m = re.match(DECLARED, line)
        if m and under:
            marked.add(m.group(1))
    assert marked == engine.CALL_TIME_SYMBOLS and isinstance(engine.CALL_TIME_SYMBOLS, frozenset)
    assert {"pf_bootstrap", "pf_resample_sites_device", "pf_forward_sites", "pf_forward_windows", "pf_window_count", "pf_window_start",
            "pf_gather_sites_device", "pf_nj_format_joins_n", "pf_bme_newick_n", "pf_bme_spr_newick_n", "pf_bionj_newick_n"} <= marked
    assert not {"pf_forward", "pf_forward_device", "pf_forward_sharded", "pf_selftest", "pf_nj_newick_n", "pf_phylip_write_batch",
                "pf_mha_forward"} & marked


def test_a_missing_function_fails_at_load_unless_its_banner_allows_it(monkeypatch):
    def library(names):
        return types.SimpleNamespace(**{n: (lambda: engine.ABI_VERSION) for n in names})      # (each its own object)
    base = set(engine.SIGNATURES) - engine.CALL_TIME_SYMBOLS
    monkeypatch.setattr(C, "CDLL", lambda path: library(base))
    lib = engine.load_library(__file__)
    assert lib.pf_forward.argtypes == engine.SIGNATURES["pf_forward"][1] and not hasattr(lib, "pf_bootstrap")
    monkeypatch.setattr(C, "CDLL", lambda path: library(base - {"pf_selftest"}))
    with pytest.raises(AttributeError, match="pf_selftest"):
        engine.load_library(__file__)


def test_a_library_without_a_symbol_raises_when_it_is_called():
    import numpy as np
    e = engine.Engine.__new__(engine.Engine)
    e._lib, e._h = types.SimpleNamespace(), None
    for call in (lambda: e.forward(np.zeros((3, 4), np.uint8)),                        # hand-written, bound at load
                 lambda: e.tree_fit_device(0, 0, 0, 1, 1, 3, 0, 0, 0, 0),             # generated
                 lambda: e.bootstrap(np.zeros((3, 4), np.uint8), 2),                   # call-time since the header says so
                 lambda: e.forward_windows(np.zeros((3, 4), np.uint8), 2)):
        with pytest.raises(engine.EngineError, match="does not export pf_"):
            call()


def test_pass_throughs_over_the_built_library_with_a_null_handle():
    """The header promises that a NULL handle is refused with nothing dereferenced: every generated method, called with
    zeros at its full arity, raises ValueError (PF_EINVAL); with one argument too few ctypes raises TypeError."""
    from phyloformer_amd import build
    build.build()
    e = engine.Engine.__new__(engine.Engine)
    e._lib, e._h = engine.load_library(), None
    assert len(engine.PASS_THROUGHS) == 19
    for name, symbol in engine.PASS_THROUGHS.items():
        method = getattr(e, name)
        assert symbol == "pf_" + name and method.__doc__ == cabi.PROTOTYPES[symbol].text and method.__name__ == name
        arity = len(engine.SIGNATURES[symbol][1]) - 1
        with pytest.raises(ValueError):
            method(*[0] * arity)
        with pytest.raises(TypeError):
            method(*[0] * (arity - 1))
