"""Process-wide settings of the HIP path: the one table of FABIND_* environment variables, and the numeric mode."""
import os
from collections import namedtuple

# Every FABIND_* environment variable the package reads.  Categories:
#   'mode-seed'   seeds the default of a numerics mode of this module's set_* API (results change; parity asserted in the GPU suite);
#   'ab'          switch between two implementations of the same arithmetic;
#   'native-dev'  handed to a setter of the native library (`setter`) by _lib.load() when set;
#   'debug'       development aids.
# attr: the module attribute (or function) the value lands in, read once at import; tests and probes assign those attributes.
# type: bool is on exactly for "1" -- `lenient` ones for everything but "0" --, int / str parse the value; an unset variable reads as
# `default` (None: the native setter is not called; there an empty value counts as unset too).  exercised_by: the test or tool that drives the non-default side of an 'ab' / 'native-dev' knob;
# one that nothing drives does not stay (tests/test_host_cpu.py).
Knob = namedtuple("Knob", "name default type category doc exercised_by attr setter lenient", defaults=(None, None, None, False))

KNOBS = {k.name: k for k in (
    Knob("FABIND_X3_WGRAD", "bf16", str, "mode-seed", "'bf16x3': anything but bf16 seeds set_x3_backward('exact') (split weight-gradient contractions)"),
    Knob("FABIND_X3_PAIRBIAS_BWD", "bf16", str, "mode-seed", "'bf16x3': anything but bf16 seeds set_x3_backward('exact') (fp32 pair-bias adjoint)"),
    Knob("FABIND_SPLIT_SITES", 3, int, "mode-seed", "'bf16': default of set_split_sites(level), 0-3"),
    Knob("FABIND_X3_EDGE", "split", str, "mode-seed", "'bf16x3': default of set_x3_edge(kind), split / bf16"),
    Knob("FABIND_ATTN_FUSED_TRAIN", True, bool, "ab", "0: the differentiable pass reads / writes [pairs, 8] bias tensors (round 3)", "tests/test_gpu_attn_mfma.py", "ops.FUSED_ATTN_TRAIN"),
    Knob("FABIND_EDGE_SAVE_FWD", True, bool, "ab", "0: the recompute backward (four contractions, nothing kept)", "tools/probes/edge_saved_forward_ab.sh", "ops.EDGE_SAVE_FWD", lenient=True),
    Knob("FABIND_FUSE_DB_TN", True, bool, "ab", "bias gradients ride along with the TN weight-gradient contraction", "tools/probes/db_tn_ab.sh", "ops.FUSE_DB_TN"),
    Knob("FABIND_INTER_ATTN_ROWS", True, bool, "ab", "0: one wave per row whatever its degree (rounds 1-4; A/B)", "tests/test_gpu_kernels.py", "kernels.INTER_ATTN_ROWS"),
    Knob("FABIND_LAYOUT_CACHE", True, bool, "ab", "0: Layout.of rebuilds the layout on every call (A/B)", "tools/probes/layout_cache_ab.sh", "engine.LAYOUT_CACHE", lenient=True),
    Knob("FABIND_PAIRHAD_ROWS", True, bool, "ab", "adjoint of the pair Hadamard as a row walk of the inter graph (no atomics)", "tools/probes/pairhad_ab.sh", "ops.PAIRHAD_ROWS"),
    Knob("FABIND_PARAM_PACK", "1", str, "ab", "0: parameter views as torch ops per entry (round 1); check: verify that no parameter element "
         "is requested twice; read at call time (param_pack())", "tests/test_gpu_param_pack.py", "config.param_pack"),
    Knob("FABIND_PLUS_FOLD_EDGE_LN", True, bool, "ab", "0: no LayerNorm-folded edge / coordinate Linears (A/B)", "tools/probes/plus_ab_samebox.sh", "plus.engine.FOLD_EDGE_LN"),
    Knob("FABIND_PLUS_FOLD_EDGE_LN_TRAIN", True, bool, "ab", "0: under autograd concat -> LayerNorm -> GEMM (rounds 1-4; A/B)", "tests/test_gpu_plus.py", "plus.engine.FOLD_EDGE_LN_TRAIN"),
    Knob("FABIND_PLUS_FUSE_PAIR", True, bool, "ab", "0: the pair update of no-grad bf16 passes as separate kernels (A/B)", "tools/probes/plus_ab_samebox.sh", "plus.engine.FUSE_PAIR"),
    Knob("FABIND_ROWS_HADAMARD_WALK", True, bool, "ab", "adjoint of rows_hadamard as a row walk (0: float atomics)", "tests/test_gpu_kernels.py", "ops.ROWS_HADAMARD_WALK"),
    Knob("FABIND_TN_DEFER", True, bool, "ab", "0: every contraction is its own launch pair (round 3's behaviour; A/B)", "tests/test_gpu_kernels.py", "kernels.TN_DEFER"),
    Knob("FABIND_EDGE_BWD3_EXP", None, int, "native-dev", "experiment mask of the store-wave backward (32 = nt operand stores)", "tools/probes/edge_bwd_nt.sh", "_lib.load", "fabind_gcl_edge_fused_bwd3_set_exp"),
    Knob("FABIND_EDGE_BWD_VARIANT", None, int, "native-dev", "form of the fused edge backward, for same-box A/B runs", "tools/probes/edge_knobs_ab.sh", "_lib.load", "fabind_gcl_edge_fused_bwd_set_variant"),
    Knob("FABIND_GEMM_SMALL_M", None, int, "native-dev", "row count below which fabind_gemm takes its small-M tile (0: never)", "tools/probes/small_m_ab.sh", "_lib.load", "fabind_gemm_set_small_m"),
    Knob("FABIND_TN_WAVES", None, int, "native-dev", "work-group layout of the TN contraction", "tools/probes/tn_layout_ab.sh", "_lib.load", "fabind_gemm_tn_set_waves"),
    Knob("FABIND_DEBUG_GRAPH", False, bool, "debug", "validate the inter-graph CSR on the host", attr="engine.DEBUG_GRAPH"),
    Knob("FABIND_DEBUG_SYNC", False, bool, "debug", "synchronise after every launch: a device fault surfaces at its launch", attr="_lib._DEBUG_SYNC"),
    Knob("FABIND_LIB", "", str, "debug", "path of the library to load instead of the built one: an A/B build (tools/probes)", attr="_lib.LIB_PATH"),
)}


def read(name, env):
    """Value of variable `name` in the mapping `env`, parsed by its declared type.  An unknown name is an error."""
    k = KNOBS[name]
    raw = env.get(name)
    if k.type is bool:
        return k.default if raw is None else (raw != "0" if k.lenient else raw == "1")
    if raw is None or (raw == "" and k.default is None):
        return k.default
    return k.type(raw)


_VALUES = {name: read(name, os.environ) for name in KNOBS}        # evaluated once, at import


def knob(name):
    return _VALUES[name]


def param_pack():
    """FABIND_PARAM_PACK as of now ('1' / '0' / 'check'): the one variable read at call time (tests/test_gpu_param_pack.py changes it)."""
    return read("FABIND_PARAM_PACK", os.environ)


def knobs_markdown():
    """The table of docs/KNOBS.md's A/B section (`python -m fabind_amd.config`)."""
    show = lambda d: "unset" if d in (None, "") else "`%s`" % (int(d) if isinstance(d, bool) else d)
    rows = ["| variable | default | file | note |", "|---|---|---|---|"]
    for k in sorted(KNOBS.values(), key=lambda k_: k_.name):
        if k.category != "mode-seed":
            where = "`fabind_amd/%s.py`" % k.attr.rsplit(".", 1)[0].replace(".", "/")
            rows.append("| `%s` | %s | %s | %s%s |" % (k.name, show(k.default), where, k.doc, " (`%s`)" % k.exercised_by if k.exercised_by else ""))
    return "\n".join(rows)


_PRECISION = {"mode": "bf16", "x3_backward": "bf16" if (knob("FABIND_X3_WGRAD") == "bf16" and knob("FABIND_X3_PAIRBIAS_BWD") == "bf16") else "exact"}
MODES = ("fp32", "bf16", "bf16x3")
_PRECISION["split_sites"] = knob("FABIND_SPLIT_SITES")


def set_precision(mode):
    """'fp32': exact-fp32 MFMA everywhere (parity mode, 1e-4 A gate; 1/16 of the bf16 matrix rate).
    'bf16': bf16 MFMA operands with fp32 accumulation; coordinates, radial terms, softmax and all
    reductions stay fp32; edge-level intermediates are stored as bf16.
    'bf16x3': fp32 storage everywhere like 'fp32'; the FORWARD pass and the activation-gradient chain of the backward pass run every
    contraction as SPLIT bf16 on the bf16 matrix cores: an operand element x is hi + lo with hi = bf16(x), lo = bf16(x - hi) (16
    significand bits), a product term is three MFMAs (lo*hi + hi*lo + hi*hi) with fp32 accumulation -- fp32-grade outputs (the mode
    that meets the 1e-4 A gate) at 3/16 of the fp32 matrix time.  Three parts of the BACKWARD pass default to single bf16 roundings of
    their fp32 operands (`set_x3_backward("bf16")`, the default): the weight-gradient contractions, the fused edge backward (the bf16
    recompute kernel on bf16 copies of AB and the weights) and the pair-bias adjoint -- parameter gradients are then bf16-grade
    (whole-gradient l2 error ~2e-3, tests/test_gpu_headline.py), the outputs and losses are not affected.
    `set_x3_backward("exact")` runs the weight gradients as split contractions, the pair-bias adjoint in fp32 and -- round 5 -- a
    differentiable pass's intra-graph edge pipeline UNFUSED (engine.gcl_layer: fp32 edge tensors, split contractions in the forward, the
    input gradients and the weight gradients; there is no split form of the fused edge backward kernel): no bf16 rounding anywhere in the
    adjoint, at the cost of ~3 GB of edge tensors per layer and the unfused launches; bench.py reports both (`gate_mode`,
    `gate_mode_exact_bwd`)."""
    assert mode in MODES
    _PRECISION["mode"] = mode


def set_split_sites(level):
    """'bf16' mode only: which node-level GEMM sites run their FORWARD contraction in split precision (three bf16 MFMAs per product term on
    the fp32 activation and the fp32 master weight, like 'bf16x3') instead of on bf16-rounded operands.  Measured at the headline shape
    (tools/probes/precision_sites.py, precision_mixed.py; profiles/r05_precision_sites.txt): of the bf16 mode's 1.0e-4 A ligand-RMSD gap to
    the fp32 reference, the bf16 edge pipeline carries 3.5e-6 and the bf16 attention tiles 1.3e-6; the node-level GEMM operand roundings
    carry the rest, and three sites most of that -- the inter-edge attention's q | k | v projection (5.4e-5 alone), its coordinate-MLP
    projection cv = Wc v (5.7e-5) and the stack's input Linear (3.2e-5).
      0: none (rounds 1-4: every GEMM on bf16 operands): 1.00e-4 / 1.76e-4 / 6.26e-4 A at n_iter 1 / 2 / 8;
      1: those three sites (9 of the ~50 node-level GEMMs of a pass): 3.84e-5 / 6.71e-5 / 2.45e-4 A (q | k | v fully split);
      2 (round 5's default): + the protein-query attention block's output projection and both blocks' k | v projections (21 GEMMs of a pass), and of
         q | k | v only the V columns (the q and k columns do not carry the gap: tools/probes/precision_qkv_parts.py):
         3.07e-5 / 4.66e-5 / 1.90e-4 A -- the 1e-4 A gate met with margin for one and two passes; headline -2.4 %, forward only -5 %.
      (Measured on MI355X: profiles/r05_precision_sites.txt.  The remaining gap sits in the GEMMs whose activation operand is a HIDDEN
      layer -- node MLP, Transition --, which the bf16 mode stores as bf16: emulated with those in split precision too the loop reads
      5.8e-5 A at n_iter 8; 'bf16x3' is the mode that meets the gate there.)
      3 (round 6, default): + both Linears of every node MLP (egnn.py:89-109) and of both Transitions (model_utils.py:162-175), with the
         hidden layer kept in fp32 between them (no-grad passes: two split-precision launches instead of the one-kernel bf16 node chain;
         under autograd the bf16 roundings of the hidden activation / its derivative are saved for the unchanged backward), the
         ligand-query block's output projection, and the full model's embedding Linears around the two stacks (models/model.py `_lin`):
         1.37e-5 / 2.73e-5 / 7.76e-5 A at n_iter 1 / 2 / 8 -- the 1e-4 A gate met in the production loop at the headline shape; config 3 read
         literally 1.6e-5 A (level 2: 5.6e-5); full IaBNet at production size, n_iter 8: stage 1 9.1e-5 A (met), stage 2 -- the ligand moves
         17 A -- 1.3e-4 A (missed; 'bf16x3' is the mode for that loop).  Cost, same box (profiles/r06_split_sites.txt): stack step -6.5 %,
         config-3 step -4 %, n_iter 8 -12 % (the four MLP contractions of a layer cost three MFMAs per product term and fp32 operands).
    Backward passes are unchanged (bf16 operands; the gradients of a bf16-mode step are bf16-grade either way)."""
    assert level in (0, 1, 2, 3)
    _PRECISION["split_sites"] = int(level)


def split_sites():
    return _PRECISION["split_sites"] if _PRECISION["mode"] == "bf16" else 0


_PRECISION["x3_edge"] = knob("FABIND_X3_EDGE")


def set_x3_edge(kind):
    """'bf16x3' mode: the fused intra-graph edge pipeline (MC_E_GCL edge / coord model, egnn.py:68-128) as
      'split' (default): the split-bf16 forward kernel on fp32 AB rows (fp32-grade node features: H to 4e-6 of its largest entry);
      'bf16'  (round 5, an option): the bf16 kernels of the 'bf16' mode on a bf16 copy of the per-node projections AB: forward 2.2 instead
               of 4.9 ms per launch -- gate mode 531 -> 592 complexes/s, the n_iter 8 loop 156 -> 202 -- and the COORDINATE / loss gates still
               met, with less margin: ligand RMSD 3.5e-6 / 7.0e-6 / 3.0e-5 A at n_iter 1 / 2 / 8 at the headline shape (split: 8e-7 / 9e-7 /
               2.9e-6), full IaBNet at production size 5.1e-5 / 2.0e-5 A (2.3e-6 / 2.6e-6); node features H to 3.4e-4 only (the messages
               are summed as bf16) -- profiles/r05_precision_sites.txt, tests/test_gpu_headline.py."""
    assert kind in ("bf16", "split")
    _PRECISION["x3_edge"] = kind


def x3_edge_bf16():
    return _PRECISION["x3_edge"] == "bf16"


# (round 6: `set_x3_attn("bf16")` -- the bf16 fused attention kernels inside the 'bf16x3' mode, +3.5 % -- is RETIRED: the full IaBNet's stage 2
#  read 9.35e-5 A with it, inside the 1e-4 A gate without margin; a switch whose on-state cannot be asserted at the gate does not ship.)


def set_x3_backward(kind):
    """'bf16' (default) / 'exact': see set_precision('bf16x3')."""
    assert kind in ("bf16", "exact")
    _PRECISION["x3_backward"] = kind


def x3_backward_bf16():
    return _PRECISION["x3_backward"] == "bf16"


def get_precision():
    return _PRECISION["mode"]


def fp32_storage():
    """True in the modes that keep every activation / weight in fp32 ('fp32' and 'bf16x3')."""
    return _PRECISION["mode"] != "bf16"


if __name__ == "__main__":
    print(knobs_markdown())
