"""The Python / C boundary, once for every header under include/ (CPU only): the ctypes signatures `posecnn_amd._lib`
derives from the prototypes are the ones installed on the loaded library, the library exports exactly what the headers
declare, every symbol has one home, and the parser's grammar is closed — what it does not know it refuses.

PINNED is the one hand-kept table: a new header, or a new entry in a header whose list is exact, needs its row here."""
import glob
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_int64, c_long, c_size_t, c_uint32, c_uint64, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
MAIN = "posecnn_hip.h"

# header -> its exact symbol list, or for the main header (which only grows) the least number of symbols
PINNED = {
    "posecnn_hip.h": 17,
    "posecnn_hip_train.h": ["pcnn_smooth_l1_vertex_gt_bwd", "pcnn_smooth_l1_vertex_gt_fwd", "pcnn_vertex_targets_fwd"],
    "posecnn_hip_frontend.h": ["pcnn_bilateral_u8c3_fwd", "pcnn_depth_normals_fwd", "pcnn_normal_image_fwd"],
    "posecnn_hip_synth.h": ["pcnn_synth_scene_fwd", "pcnn_synth_scene_workspace_bytes"],
    "posecnn_hip_augment.h": ["pcnn_augment_frames_fwd", "pcnn_augment_frames_workspace_bytes"],
    "posecnn_hip_loss.h": ["pcnn_label_head_loss_bwd", "pcnn_label_head_loss_fwd", "pcnn_label_head_loss_workspace_bytes"],
    "posecnn_hip_vertex_loss.h": ["pcnn_vertex_head_loss_bwd", "pcnn_vertex_head_loss_fwd", "pcnn_vertex_head_loss_workspace_bytes"],
    "posecnn_hip_trunk_train.h": ["pcnn_bias_relu_pool2_train_bwd", "pcnn_bias_relu_pool2_train_fwd",
                                  "pcnn_bias_relu_pool2_train_workspace_bytes", "pcnn_bias_relu_train_bwd",
                                  "pcnn_bias_relu_train_workspace_bytes"],
    "posecnn_hip_pose3d.h": ["pcnn_pose3d_estimate_fwd", "pcnn_pose3d_prepare_fwd", "pcnn_pose3d_round_fwd", "pcnn_pose3d_sample_fwd",
                             "pcnn_pose3d_workspace_bytes"],
    "posecnn_hip_pose2d.h": ["pcnn_pose2d_estimate_fwd", "pcnn_pose2d_prepare_fwd", "pcnn_pose2d_round_fwd", "pcnn_pose2d_sample_fwd",
                             "pcnn_pose2d_workspace_bytes"],
    "posecnn_hip_wino_packed.h": ["pcnn_winograd43_conv_packed_fwd", "pcnn_winograd43_pack_filters_fwd"],
}

# the headers that do not include posecnn_hip.h (they use none of its names); every other one, a new one too, must
SELF_CONTAINED = {"posecnn_hip_pose3d.h", "posecnn_hip_pose2d.h", "posecnn_hip_wino_packed.h"}


@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _text(header):
    """The header without its block comments, as the per-header tests before this one read it."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


# ---- the headers against the loaded library --------------------------------------------------------------------------
@pytest.mark.parametrize("header", HEADERS)
def test_header_is_bound_as_declared(L, header):
    from posecnn_amd import _lib
    table = _lib.BINDINGS[header]
    text = _text(header)
    # the symbols, found without the parser
    syms = sorted(set(re.findall(r"\b(pcnn_[a-z0-9_]+)\s*\(", text)))
    assert sorted(table) == syms
    assert header in PINNED, "tests/test_capi_bindings.py pins no symbol list for %s" % header
    if header == MAIN:
        assert len(syms) >= PINNED[header]
        assert "pcnn_pose2d_" not in open(os.path.join(ROOT, "include", header)).read()      # that route has its own header
    else:
        assert syms == PINNED[header]
    for s in syms:
        fn = getattr(L, s)                                       # AttributeError: not exported
        assert fn.restype is table[s][0], s
        assert list(fn.argtypes) == table[s][1], s
        # one ctypes type per parameter of the declaration, counted without the parser
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text).group(1)
        assert len(fn.argtypes) == (0 if decl.strip() == "void" else len(decl.split(","))), s
    if header != MAIN:
        # one ABI version, the main header's; the three SELF_CONTAINED headers take nothing from it and include only libc's
        assert "PCNN_ABI_VERSION" not in text
        includes = re.findall(r"^#include (\S+)$", text, flags=re.M)
        assert includes == (["<stddef.h>", "<stdint.h>"] if header in SELF_CONTAINED else ['"posecnn_hip.h"'])


def test_abi_version_is_the_headers(L):
    from posecnn_amd import _lib
    version = int(re.search(r"^#define PCNN_ABI_VERSION (\d+)$", _text(MAIN), flags=re.M).group(1))
    assert _lib.header_abi_version() == version == L.pcnn_abi_version() == 2


def test_library_exports_exactly_the_declared_symbols(L):
    from posecnn_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] in "Tt" and f[2].startswith("pcnn_"))
    declared = sorted(s for table in _lib.BINDINGS.values() for s in table)
    assert exported == declared
    assert len(declared) == len(set(declared)) >= 101             # one home per symbol; the count when this test was written


def test_each_symbol_has_one_header():
    seen = {}
    for header in HEADERS:
        for s in set(re.findall(r"\b(pcnn_[a-z0-9_]+)\s*\(", _text(header))):
            assert s not in seen, "%s is declared in %s and %s" % (s, seen[s], header)
            seen[s] = header
    assert sorted(PINNED) == HEADERS


def test_ops_export_the_training_heads():
    from posecnn_amd import ops
    for name in ("label_head_loss", "label_head_loss_grad", "vertex_head_loss", "vertex_head_loss_grad"):
        assert name in ops.__all__


# ---- the parser on literal text ----------------------------------------------------------------------------------------
P = c_void_p
FORMS = [
    ("int pcnn_a(void);", c_int, []),
    ("const char* pcnn_a(int status);", c_char_p, [c_int]),
    ("const char *pcnn_a(void);", c_char_p, []),
    ("long pcnn_a(char* buf, long cap);", c_long, [c_char_p, c_long]),
    ("uint32_t pcnn_a(const void* data, size_t num_bytes, uint32_t seed);", c_uint32, [P, c_size_t, c_uint32]),
    ("int pcnn_a(float x, int64_t n, uint64_t key, const char* name);", c_int, [c_float, c_int64, c_uint64, c_char_p]),
    ("int pcnn_a(size_t* bytes, int* num_counters, const int* other);", c_int, [POINTER(c_size_t), POINTER(c_int), POINTER(c_int)]),
    ("int pcnn_a(const float* x, float *y, int32_t* label, const int32_t* gt, const uint8_t* c, const uint16_t* d, uint8_t* m);",
     c_int, [P] * 7),
    ("int pcnn_a(const double* means, double* update, void* workspace, const void* data, void* stream);", c_int, [P] * 5),
    ("int pcnn_a(int, float, const float*, size_t*);", c_int, [c_int, c_float, P, POINTER(c_size_t)]),   # unnamed parameters
]


@pytest.mark.parametrize("text,restype,argtypes", FORMS, ids=[f[0][:40] for f in FORMS])
def test_parser_maps_every_supported_form(text, restype, argtypes):
    from posecnn_amd import _lib
    assert _lib.parse_header("t.h", text) == {"pcnn_a": (restype, argtypes)}


def test_parser_reads_prototypes_not_comments():
    from posecnn_amd import _lib
    text = """
        #ifndef T_H_
        #define T_H_
        #include "posecnn_hip.h"
        #define PCNN_T_ROWS (PCNN_MAX_ROI * 9)
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef enum pcnn_t { PCNN_T_A = 0 } pcnn_t;
        /* int pcnn_in_a_block_comment(int a);
         * spread over lines: int pcnn_also_not(void); */
        // int pcnn_behind_slashes(float x);
        int pcnn_first(const float* x,   /* an input */
                       int batch,        // how many
                       size_t*
                           bytes);
        const char*
        pcnn_second(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """
    got = _lib.parse_header("t.h", text)
    assert list(got) == ["pcnn_first", "pcnn_second"]
    assert got["pcnn_first"] == (c_int, [P, c_int, POINTER(c_size_t)]) and got["pcnn_second"] == (c_char_p, [])


REFUSED = [
    ("int pcnn_a(unsigned long long n);", r"t\.h: pcnn_a: parameter 1 'unsigned long long n'"),
    ("int pcnn_a(int n, float** rows);", r"t\.h: pcnn_a: parameter 2 'float\*\* rows'.*pointer to pointer"),
    ("int pcnn_a(float rows[4]);", r"t\.h: pcnn_a: parameter 1 'float rows\[4\]'"),
    ("int pcnn_a(int n, void (*done)(int, void*));", r"t\.h: pcnn_a: parameter 2 'void \(\*done\)\(int, void\*\)'"),
    ("float pcnn_a(int n);", r"t\.h: pcnn_a: return type 'float'"),
    ("struct pcnn_t* pcnn_a(void);", r"t\.h: pcnn_a: return type"),
    ("int pcnn_a(double x);", r"t\.h: pcnn_a: parameter 1 'double x'"),
    ("int pcnn_a(int n);\nint pcnn_a(int n);", r"t\.h: pcnn_a is declared twice"),
    ("static inline int pcnn_a(int n) { return n; }", r"t\.h: pcnn_a: not a prototype"),
]


@pytest.mark.parametrize("text,message", REFUSED, ids=[r[0][:32] for r in REFUSED])
def test_parser_refuses_what_is_outside_the_grammar(text, message):
    from posecnn_amd import _lib
    with pytest.raises(ValueError, match=message):
        _lib.parse_header("t.h", text)


def test_parser_refuses_a_symbol_in_two_headers():
    from posecnn_amd import _lib
    one, two = "int pcnn_a(int n);", "int pcnn_b(void);\nint pcnn_a(int n);"
    assert list(_lib.parse_headers([("one.h", one), ("two.h", "int pcnn_b(void);")])) == ["one.h", "two.h"]
    with pytest.raises(ValueError, match=r"two\.h: pcnn_a is already declared in one\.h"):
        _lib.parse_headers([("one.h", one), ("two.h", two)])
