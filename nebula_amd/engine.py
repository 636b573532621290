"""Host-side mirror of the reference's GetNeighbors / GO interface over libnebula_gn.so.

`Engine` is one shard (one GPU). Its methods follow the reference call surface for the path:
  add_space / add_schema   meta::SchemaManager (src/meta/SchemaManager.h:18-56)
  load_kv / commit         the KV rows of the space's parts (NebulaKeyUtils keys + RowWriter values)
                           -> per-part CSR + columnar props in HBM
  get_neighbors            StorageClient::getNeighbors -> QueryBoundProcessor
                           (src/storage/client/StorageClient.cpp:121-157, QueryBoundProcessor.cpp)
  go                       GoExecutor (src/graph/GoExecutor.cpp) for `GO [M TO] N STEPS FROM ...
                           OVER ... [REVERSELY|BIDIRECT] [WHERE ...] YIELD [DISTINCT] ...`
There is no CPU fallback: a missing library raises at import of the first Engine.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import ngql

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnebula_gn.so")

NGX_OK = 0
E_BAD_ARGUMENT = -1001
E_UNSUPPORTED = -1002
E_QUERY = -1003
E_DEVICE = -1004
E_NOT_LOADED = -1005
E_SNAPSHOT = -1006

SOURCE, DEST, EDGE = 1, 2, 3


class EngineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{code}] {msg}")
        self.code = code


# ----------------------------------------------------------------------------- C structs
c_i32, c_i64, c_u32, c_u64, c_dbl = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
P = ctypes.POINTER


class Config(ctypes.Structure):
    _fields_ = [("device", c_i32), ("rank", c_i32), ("world", c_i32), ("nccl_unique_id", ctypes.c_void_p),
                ("exchange", ctypes.c_void_p), ("exchange_user", ctypes.c_void_p)]


class KVBatchC(ctypes.Structure):
    _fields_ = [("n", c_u64), ("keys", ctypes.c_void_p), ("key_off", ctypes.c_void_p), ("vals", ctypes.c_void_p),
                ("val_off", ctypes.c_void_p)]


class GraphInfo(ctypes.Structure):
    _fields_ = [("vertices", c_u64), ("edges", c_u64), ("device_bytes", c_u64), ("slots", c_i32), ("tags", c_i32)]


class CellV(ctypes.Union):
    _fields_ = [("i", c_i64), ("d", c_dbl), ("str_off", c_u64)]


class Cell(ctypes.Structure):
    _fields_ = [("kind", c_i32), ("str_len", c_i32), ("v", CellV)]


class PropDef(ctypes.Structure):
    _fields_ = [("owner", c_i32), ("id", c_i32), ("name", ctypes.c_char_p)]


class GnRequest(ctypes.Structure):
    _fields_ = [("space", c_i32), ("nparts", c_i32), ("parts", P(c_i32)), ("part_nvids", P(c_u32)),
                ("vids", P(c_i64)), ("nedge_types", c_i32), ("edge_types", P(c_i32)), ("filter", ctypes.c_char_p),
                ("filter_len", c_u32), ("ncols", c_i32), ("cols", P(PropDef)), ("max_edges_per_vertex", c_i32),
                ("now_sec", c_i64), ("encode_rows", c_i32)]


class SchemaDefC(ctypes.Structure):
    _fields_ = [("is_edge", c_i32), ("id", c_i32), ("ncols", c_i32), ("names", P(ctypes.c_char_p)),
                ("types", P(c_i32))]


class GnResult(ctypes.Structure):
    _fields_ = [("code", c_i32), ("nfailed", c_i32), ("failed_codes", P(c_i32)), ("nedges", c_u64),
                ("edge_vertex", P(c_u32)), ("edge_type", P(c_i32)), ("edge_dst", P(c_i64)), ("ncols", c_i32),
                ("edge_cells", P(Cell)), ("nvertices", c_u32), ("vertex_cells", P(Cell)),
                ("vertex_has_tag", P(ctypes.c_uint8)), ("strings", ctypes.c_void_p), ("strings_len", c_u64),
                ("edge_props", ctypes.c_void_p), ("edge_props_off", P(c_u64)), ("nschemas", c_i32),
                ("schemas", P(SchemaDefC)), ("ntag_rows", c_u32), ("tag_row_vertex", P(c_u32)),
                ("tag_row_tag", P(c_i32)), ("tag_props", ctypes.c_void_p), ("tag_props_off", P(c_u64)),
                ("latency_in_us", c_i64)]


class GoPlan(ctypes.Structure):
    _fields_ = [("space", c_i32), ("record_from", c_u32), ("record_to", c_u32), ("nstarts", c_u64),
                ("starts", P(c_i64)), ("nover", c_i32), ("over_names", P(ctypes.c_char_p)),
                ("over_aliases", P(ctypes.c_char_p)), ("over_all", c_i32), ("direction", c_i32),
                ("where", ctypes.c_char_p), ("where_len", c_u32), ("nyields", c_i32),
                ("yields", P(ctypes.c_char_p)), ("yield_lens", P(c_u32)), ("distinct", c_i32),
                ("filter_pushdown", c_i32), ("now_sec", c_i64), ("result_on_device", c_i32),
                ("host_columnar", c_i32), ("input_vid_col", ctypes.c_char_p), ("input_var", ctypes.c_char_p),
                ("input_ncols", c_i32), ("input_names", P(ctypes.c_char_p)), ("input_types", P(c_i32)),
                ("input_nrows", c_u64), ("input_cells", P(Cell)), ("input_strings", ctypes.c_char_p),
                ("yield_only", c_i32), ("compact_results", c_i32)]


_CELL_KIND = {"empty": 0, "bool": 1, "int": 2, "id": 3, "float": 4, "double": 5, "str": 6, "timestamp": 21}


def _input_arrays(inp):
    """An Interim (nebula_amd.pipeline) as the plan's input_* arrays; the tuple keeps them alive."""
    nc, nr = len(inp.names), len(inp.rows)
    names = (ctypes.c_char_p * max(1, nc))(*[n.encode() for n in inp.names])
    types = (c_i32 * max(1, nc))(*(list(inp.types) + [0] * (nc - len(inp.types))))
    cells = (Cell * max(1, nr * nc))()
    strings = bytearray()
    for r, row in enumerate(inp.rows):
        for c, (kind, v) in enumerate(row):
            cl = cells[r * nc + c]
            cl.kind = _CELL_KIND[kind] if not (kind == "empty" and v is not None) else 1
            if kind == "str":
                b = v.encode("utf-8", "surrogateescape")
                cl.v.str_off = len(strings)
                cl.str_len = len(b)
                strings += b
            elif kind in ("float", "double"):
                cl.v.d = v
            elif v is not None:                                   # ints, bools (an unset bool too)
                cl.v.i = int(v)
    return names, types, cells, bytes(strings) + b"\0", nc, nr


class CsrSlotC(ctypes.Structure):
    _fields_ = [("etype", c_i32), ("off", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("rank", ctypes.c_void_p),
                ("ncols", c_i32), ("cols", ctypes.c_void_p)]


class CsrShardC(ctypes.Structure):
    _fields_ = [("nvertices", c_u64), ("vpart", ctypes.c_void_p), ("vid", ctypes.c_void_p), ("nslots", c_i32),
                ("slots", P(CsrSlotC))]


class GoResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("ncols", c_i32), ("col_types", P(c_i32)), ("nrows", c_u64), ("cells", P(Cell)),
                ("row_src", P(c_i64)), ("row_dst", P(c_i64)), ("row_rank", P(c_i64)), ("row_type", P(c_i32)),
                ("strings", ctypes.c_void_p), ("strings_len", c_u64), ("nhops", c_i32),
                ("hop_frontier", P(c_u64)), ("hop_edges", P(c_u64)), ("hop_next", P(c_u64)),
                ("device_ms", c_dbl), ("dev_src", ctypes.c_void_p), ("dev_dst", ctypes.c_void_p),
                ("dev_rank", ctypes.c_void_p), ("dev_type", ctypes.c_void_p), ("dev_cols", ctypes.c_void_p),
                ("dev_type_const", ctypes.c_int32), ("host_cols", ctypes.c_void_p),
                ("hop_exchange_bytes", P(c_u64)), ("host_prep_ms", c_dbl), ("host_tail_ms", c_dbl),
                ("dev_key_w", c_i32 * 3), ("dev_col_w", P(c_i32)),
                ("dev_key_const", c_i64 * 3), ("dev_col_const", P(c_i64))]


AGG_FN = {"": 0, "COUNT": 1, "COUNT_DISTINCT": 2, "SUM": 3, "AVG": 4, "MAX": 5, "MIN": 6, "STD": 7, "BIT_AND": 8,
          "BIT_OR": 9, "BIT_XOR": 10}                              # NGX_AGG_*


class AggColC(ctypes.Structure):
    _fields_ = [("fn", c_i32), ("col", c_i32), ("konst", Cell)]


class GroupPlanC(ctypes.Structure):
    _fields_ = [("nkeys", c_i32), ("key_cols", P(c_i32)), ("nyields", c_i32), ("yields", P(AggColC))]


class GroupResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("ncols", c_i32), ("col_types", P(c_i32)), ("ngroups", c_u64), ("cells", P(Cell)),
                ("strings", ctypes.c_void_p), ("strings_len", c_u64), ("device_ms", c_dbl)]


@dataclass
class GroupBySpec:
    """ngx_group_plan: key columns and yield columns (function name, GO YIELD column or -1, constant) by
    GO YIELD index. A constant is an int, a float, or "*"."""
    key_cols: List[int]
    yields: List[Tuple[str, int, object]]


class OrderFactorC(ctypes.Structure):
    _fields_ = [("col", c_i32), ("desc", c_i32)]


class OrderPlanC(ctypes.Structure):
    _fields_ = [("nfactors", c_i32), ("factors", P(OrderFactorC)), ("offset", c_i64), ("count", c_i64)]


class OrderResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("ncols", c_i32), ("col_types", P(c_i32)), ("nrows", c_u64), ("cells", P(Cell)),
                ("strings", ctypes.c_void_p), ("strings_len", c_u64), ("input_rows", c_u64), ("device_ms", c_dbl),
                ("host_sort_ms", c_dbl)]


@dataclass
class OrderBySpec:
    """ngx_order_plan: (GO YIELD column, descending) per ORDER BY factor (none: LIMIT alone), and the LIMIT's
    offset and count (count < 0: no LIMIT, which the library refuses)."""
    factors: List[Tuple[int, bool]]
    offset: int = 0
    count: int = -1


SET_OP = {"UNION": 0, "INTERSECT": 1, "MINUS": 2, "UNION ALL": 3}    # NGX_SET_* (UNION: DISTINCT)


class SetPlanC(ctypes.Structure):
    _fields_ = [("op", c_i32)]


class SetResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("ncols", c_i32), ("col_types", P(c_i32)), ("nrows", c_u64), ("cells", P(Cell)),
                ("strings", ctypes.c_void_p), ("strings_len", c_u64), ("left_rows", c_u64), ("right_rows", c_u64),
                ("device_ms", c_dbl)]


PATH_KIND = {"SHORTEST": 0, "ALL": 1, "NOLOOP": 2}               # NGX_PATH_*


class PathPlanC(ctypes.Structure):
    _fields_ = [("space", c_i32), ("kind", c_i32), ("nfrom", c_u64), ("from_", P(c_i64)), ("nto", c_u64), ("to", P(c_i64)),
                ("nover", c_i32), ("over_names", P(ctypes.c_char_p)), ("over_all", c_i32), ("direction", c_i32), ("upto", c_u32)]


class PathResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("nedge_names", c_i32), ("edge_names", P(ctypes.c_char_p)), ("edge_types", P(c_i32)),
                ("nedges", c_u64), ("src", P(c_i64)), ("dst", P(c_i64)), ("type", P(c_i32)), ("rank", P(c_i64)),
                ("mask", P(c_u64)), ("found", c_u64), ("levels", c_i32), ("device_ms", c_dbl), ("layer", P(ctypes.c_uint8))]


FETCH_VERTEX, FETCH_EDGE = 0, 1                                 # NGX_FETCH_*
FY_TAG_PROP, FY_EDGE_PROP, FY_EDGE_KEY, FY_INPUT_COL = 0, 1, 2, 3  # NGX_FY_*
EDGE_KEY = {"_src": 0, "_dst": 1, "_rank": 2, "_type": 3}        # NGX_EK_*


class FetchYieldC(ctypes.Structure):
    _fields_ = [("kind", c_i32), ("tag", c_i32), ("field", ctypes.c_char_p), ("key", c_i32), ("col", c_i32)]


class FetchPlanC(ctypes.Structure):
    _fields_ = [("space", c_i32), ("kind", c_i32), ("ntags", c_i32), ("tags", P(c_i32)), ("edge_type", c_i32),
                ("key_cols", c_i32 * 3), ("nkeys", c_u64), ("key_vid", P(c_i64)), ("key_dst", P(c_i64)),
                ("key_rank", P(c_i64)), ("distinct", c_i32), ("keep_missing", c_i32), ("nyields", c_i32),
                ("yields", P(FetchYieldC))]


class FetchResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("ncols", c_i32), ("col_types", P(c_i32)), ("nrows", c_u64), ("cells", P(Cell)),
                ("strings", ctypes.c_void_p), ("strings_len", c_u64), ("input_rows", c_u64), ("tags_seen", c_u32),
                ("device_ms", c_dbl)]


@dataclass
class FetchSpec:
    """ngx_fetch_plan of a prepared FETCH sentence, and what fetch.device_rows needs to name, type and trim the
    device's rows as the host path would (fetch.device_spec builds it from a sentence).
    yields: (NGX_FY_*, tag id, field, NGX_EK_*, input column); kind -1: an expression the device refuses."""
    kind: int
    tags: List[int]
    edge_type: int
    key_cols: Tuple[int, int, int]
    keys: Optional[List[np.ndarray]]                              # host key arrays; None: the keys are a result's columns
    distinct: bool
    keep_missing: bool
    yields: List[Tuple[int, int, str, int, int]]
    names: List[str]
    types: List[int]                                              # schema types of every output column (0: from the value)
    yield_tag: List[int] = field(default_factory=list)            # no YIELD: index into tags of each yield's tag
    no_yield: bool = False
    prefix: List[str] = field(default_factory=list)               # the names when nothing comes back


class LookupCondC(ctypes.Structure):
    _fields_ = [("field", ctypes.c_char_p), ("kind", c_i32), ("op", c_i32), ("lo", c_u64), ("hi", c_u64),
                ("bits", c_i64), ("str", ctypes.c_char_p), ("str_len", c_u64)]


class LookupPlanC(ctypes.Structure):
    _fields_ = [("space", c_i32), ("is_edge", c_i32), ("schema_id", c_i32), ("nfields", c_i32),
                ("fields", P(LookupCondC)), ("nterms", c_i32), ("terms", P(LookupCondC)), ("nyields", c_i32),
                ("yields", P(ctypes.c_char_p))]


class LookupResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("ncols", c_i32), ("col_types", P(c_i32)), ("nrows", c_u64), ("cells", P(Cell)),
                ("strings", ctypes.c_void_p), ("strings_len", c_u64), ("scanned_rows", c_u64), ("keep_bytes", c_u64),
                ("device_ms", c_dbl)]


@dataclass
class LookupSpec:
    """ngx_lookup_plan of a planned LOOKUP sentence (lookup.device_spec builds it from a lookup.Plan), and the names
    and schema types lookup.device_rows gives the rows.
    fields / terms: (field, NGX_LK_* of the constant, operator, lo, hi, bits, string bytes)."""
    is_edge: bool
    schema_id: int
    fields: List[Tuple[str, int, int, int, int, int, bytes]]
    terms: List[Tuple[str, int, int, int, int, int, bytes]]
    yields: List[str]
    names: List[str]
    types: List[int]


class YieldColC(ctypes.Structure):
    _fields_ = [("fn", c_i32), ("expr", ctypes.c_char_p), ("expr_len", c_u32)]


class YieldPlanC(ctypes.Structure):
    _fields_ = [("ncols_in", c_i32), ("input_names", P(ctypes.c_char_p)), ("where", ctypes.c_char_p),
                ("where_len", c_u32), ("nyields", c_i32), ("yields", P(YieldColC))]


class YieldResultC(ctypes.Structure):
    _fields_ = [("code", c_i32), ("ncols", c_i32), ("col_types", P(c_i32)), ("nrows", c_u64), ("input_rows", c_u64),
                ("kept_rows", c_u64), ("cells", P(Cell)), ("strings", ctypes.c_void_p), ("strings_len", c_u64),
                ("device_ms", c_dbl)]


@dataclass
class YieldSpec:
    """ngx_yield_plan: the `$-` schema (the GO's YIELD column names), WHERE's Expression::encode bytes (None: no
    WHERE) and per yield column its function name ("" for none) and its expression's bytes."""
    input_names: List[str]
    where: Optional[bytes]
    yields: List[Tuple[str, bytes]]


class Stat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("value", c_i64)]


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("launches", c_u32), ("total_ms", c_dbl), ("algo_bytes", c_u64)]


# every symbol include/nebula_gn.h declares: (name, restype, argtypes)
SIGNATURES = {
    "ngx_open": (c_i32, [P(Config), P(ctypes.c_void_p)]),
    "ngx_close": (None, [ctypes.c_void_p]),
    "ngx_last_error": (ctypes.c_char_p, [ctypes.c_void_p]),
    "ngx_build_info": (ctypes.c_char_p, []),
    "ngx_get_unique_id": (c_i32, [ctypes.c_void_p]),
    "ngx_add_space": (c_i32, [ctypes.c_void_p, c_i32, c_i32]),
    "ngx_add_schema": (c_i32, [ctypes.c_void_p, c_i32, c_i32, c_i32, ctypes.c_char_p, c_i64, c_i32,
                               P(ctypes.c_char_p), P(c_i32), ctypes.c_char_p, c_i64]),
    "ngx_load_kv": (c_i32, [ctypes.c_void_p, c_i32, P(KVBatchC)]),
    "ngx_load_csr": (c_i32, [ctypes.c_void_p, c_i32, P(CsrShardC)]),
    "ngx_commit": (c_i32, [ctypes.c_void_p, c_i32]),
    "ngx_graph_info_get": (c_i32, [ctypes.c_void_p, c_i32, P(GraphInfo)]),
    "ngx_get_neighbors": (c_i32, [ctypes.c_void_p, P(GnRequest), P(P(GnResult))]),
    "ngx_gn_result_free": (None, [P(GnResult)]),
    "ngx_go": (c_i32, [ctypes.c_void_p, P(GoPlan), P(P(GoResultC))]),
    "ngx_go_result_free": (None, [P(GoResultC)]),
    "ngx_go_batch": (c_i32, [ctypes.c_void_p, ctypes.c_void_p, c_i32, P(c_i32), P(c_u64), P(c_u64), P(c_u64)]),
    "ngx_set_profiling": (c_i32, [ctypes.c_void_p, c_i32]),
    "ngx_synchronize": (c_i32, [ctypes.c_void_p]),
    "ngx_go_result_digest": (c_i32, [ctypes.c_void_p, P(GoResultC), P(c_u64)]),
    "ngx_go_group_by": (c_i32, [ctypes.c_void_p, P(GoResultC), P(GroupPlanC), P(P(GroupResultC))]),
    "ngx_group_result_free": (None, [P(GroupResultC)]),
    "ngx_go_order_by": (c_i32, [ctypes.c_void_p, P(GoResultC), P(OrderPlanC), P(P(OrderResultC))]),
    "ngx_order_result_free": (None, [P(OrderResultC)]),
    "ngx_go_group_order_by": (c_i32, [ctypes.c_void_p, P(GoResultC), P(GroupPlanC), P(OrderPlanC), P(P(OrderResultC))]),
    "ngx_set_op": (c_i32, [ctypes.c_void_p, P(GoResultC), P(GoResultC), P(SetPlanC), P(P(SetResultC))]),
    "ngx_go_set": (c_i32, [ctypes.c_void_p, P(GoPlan), P(GoPlan), P(SetPlanC), P(P(SetResultC))]),
    "ngx_set_result_free": (None, [P(SetResultC)]),
    "ngx_fetch": (c_i32, [ctypes.c_void_p, P(GoResultC), P(FetchPlanC), P(P(FetchResultC))]),
    "ngx_go_fetch": (c_i32, [ctypes.c_void_p, P(GoPlan), P(FetchPlanC), P(P(FetchResultC))]),
    "ngx_fetch_result_free": (None, [P(FetchResultC)]),
    "ngx_lookup": (c_i32, [ctypes.c_void_p, P(LookupPlanC), P(P(LookupResultC))]),
    "ngx_lookup_result_free": (None, [P(LookupResultC)]),
    "ngx_go_yield": (c_i32, [ctypes.c_void_p, P(GoResultC), P(YieldPlanC), P(P(YieldResultC))]),
    "ngx_yield_result_free": (None, [P(YieldResultC)]),
    "ngx_find_path": (c_i32, [ctypes.c_void_p, P(PathPlanC), P(P(PathResultC))]),
    "ngx_path_result_free": (None, [P(PathResultC)]),
    "ngx_stats": (c_i32, [ctypes.c_void_p, P(P(Stat)), P(c_i32)]),
    "ngx_kernel_stats": (c_i32, [ctypes.c_void_p, P(P(KernelStat)), P(c_i32)]),
    "ngx_set_flag": (c_i32, [ctypes.c_void_p, ctypes.c_char_p, c_i64]),
    "ngx_get_flag": (c_i32, [ctypes.c_void_p, ctypes.c_char_p, P(c_i64)]),
    "ngx_jit_note": (ctypes.c_char_p, [ctypes.c_void_p]),
    "ngx_hash_string": (c_i64, [ctypes.c_char_p, c_u64]),
    "ngx_device_to_host": (c_i32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_u64]),
    "ngx_load_snapshot_rows": (c_i32, [ctypes.c_void_p, c_i32, ctypes.c_void_p, c_u64]),
    "ngx_save_snapshot": (c_i32, [ctypes.c_void_p, c_i32, ctypes.c_char_p, ctypes.c_char_p]),
    "ngx_open_snapshot": (c_i32, [ctypes.c_void_p, c_i32, ctypes.c_char_p, ctypes.c_char_p]),
}


class DevColumn(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("len", ctypes.c_void_p), ("type", ctypes.c_void_p)]

_lib = None


def lib():
    """Load libnebula_gn.so. Raises if it is not built: there is no other implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(E_DEVICE, f"{LIB_PATH} is missing; build it with `make -C nebula_amd/csrc`")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


XCHG_ALLGATHER, XCHG_ALLTOALL = 0, 1
ExchangeFn = ctypes.CFUNCTYPE(c_i32, ctypes.c_void_p, c_i32, ctypes.c_void_p, ctypes.c_void_p, c_u64)


def dist_exchange(group=None):
    """Host collective for ngx_config.exchange over torch.distributed (gloo): lets world > 1 shards
    share one GPU (multi-shard tests) where RCCL needs one GPU per rank. Semantics: nebula_gn.h."""
    import torch
    import torch.distributed as dist

    def fn(user, op, send, recv, nbytes):
        try:
            w, me = dist.get_world_size(group), dist.get_rank(group)
            n_send = nbytes if op == XCHG_ALLGATHER else nbytes * w
            sb = torch.frombuffer(bytearray(ctypes.string_at(send, n_send)), dtype=torch.uint8) if n_send else \
                torch.zeros(0, dtype=torch.uint8)
            got = [torch.empty(n_send, dtype=torch.uint8) for _ in range(w)]
            dist.all_gather(got, sb, group=group)     # gloo has no all_to_all: gather and pick blocks
            if op == XCHG_ALLTOALL:
                got = [g[me * nbytes:(me + 1) * nbytes] for g in got]
            out = torch.cat(got).numpy()
            if out.size:
                ctypes.memmove(recv, out.ctypes.data, out.size)
            return 0
        except Exception:                          # never raise through the C ABI
            return 1

    return ExchangeFn(fn)


def unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    rc = lib().ngx_get_unique_id(buf)
    if rc:
        raise EngineError(rc, "ncclGetUniqueId failed")
    return buf.raw


# ----------------------------------------------------------------------------- results
def _cells(cells, n, ncols, strings: bytes):
    out = []
    kinds = {0: "empty", 1: "bool", 2: "int", 3: "id", 4: "float", 5: "double", 6: "str", 21: "timestamp"}
    for r in range(n):
        row = []
        for c in range(ncols):
            cl = cells[r * ncols + c]
            k = kinds.get(cl.kind, str(cl.kind))
            if cl.kind == 0:
                row.append(("empty", bool(cl.v.i) if cl.str_len == 1 else None))
            elif cl.kind == 1:
                row.append(("bool", bool(cl.v.i)))
            elif cl.kind in (4, 5):
                row.append((k, cl.v.d))
            elif cl.kind == 6:
                o = cl.v.str_off
                row.append(("str", strings[o:o + cl.str_len].decode("utf-8", "surrogateescape")))
            else:
                row.append((k, cl.v.i))
        out.append(tuple(row))
    return out


@dataclass
class GoResult:
    ok: bool
    error: str
    code: int
    col_types: List[int]
    rows: List[tuple]
    src: np.ndarray = None
    dst: np.ndarray = None
    rank: np.ndarray = None
    etype: np.ndarray = None
    hop_frontier: List[int] = field(default_factory=list)
    hop_edges: List[int] = field(default_factory=list)
    hop_next: List[int] = field(default_factory=list)
    hop_xchg: List[int] = field(default_factory=list)     # world > 1: frontier bytes sent per hop
    device_ms: float = 0.0
    nrows: int = 0
    # on_device + fetch: the HBM result copied back as arrays (x, len or None, type or None) per column
    dev_cols: List[tuple] = field(default_factory=list)
    # on_device: ([src, dst, rank] widths, per-column widths) in bytes; 8 unless compact
    dev_widths: Optional[tuple] = None
    dev_consts: Optional[tuple] = None       # (key values, column values) of width-0 (constant) columns
    digests: object = None               # columnar + digest_fn: whatever digest_fn returned
    device_digest: Optional[tuple] = None  # on_device + device_digest: (sum, xor, rows) of the row hashes
    host_prep_ms: float = 0.0            # library host time before the first launch / after the device
    host_tail_ms: float = 0.0
    # group_by: the traversal's device time and row count, and the grouping's device time
    go_device_ms: float = 0.0
    go_nrows: int = 0
    group_device_ms: float = 0.0
    # order_by: the selection's device time and the library's host sort of the winners (go_* as for group_by)
    order_device_ms: float = 0.0
    order_host_sort_ms: float = 0.0
    ngroups: int = 0                     # group_by + order_by: the groups the window was cut from
    path_found: int = 0                  # find_path: bit j set when target j was found (ngx_path_result.found)
    tags_seen: int = 0                   # fetch: bit t set when some key had a row of the plan's tag t
    keep_bytes: int = 0                  # lookup: bytes the keep pass had to read
    # yield_by: the sentence's device time, and the rows WHERE kept (go_* as for group_by)
    yield_device_ms: float = 0.0
    kept_rows: int = 0
    yield_cells: object = None           # yield_by with rows=False: the cells as a numpy (nrows, ncols) record array


@dataclass
class NeighborsResult:
    code: int
    failed_codes: List[Tuple[int, int]]
    total_edges: int
    edge_vertex: np.ndarray
    edge_type: np.ndarray
    edge_dst: np.ndarray
    edge_cells: List[tuple]
    vertex_cells: List[tuple]
    vertex_has_tag: np.ndarray
    # encode_rows: the QueryResponse payload (RowWriter rows, schemas)
    edge_props: Optional[List[bytes]] = None           # IdAndProp.props per returned edge
    edge_schema: Optional[dict] = None                 # signed type -> [(name, type)]
    vertex_schema: Optional[dict] = None               # tag id -> [(name, type)]
    tag_rows: Optional[List[Tuple[int, int, bytes]]] = None   # (request vid index, tag id, TagData.data)
    latency_in_us: int = 0                             # ResponseCommon.latency_in_us


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


# ----------------------------------------------------------------------------- engine
class PreparedGo:
    """A GO sentence encoded once for ngx_go (ngx_go_plan and the arrays it points into); reusable across
    calls while the sentence object it came from is not changed (Engine.prepare_go)."""

    def __init__(self, plan, keep):
        self.plan = plan
        self._keep = keep


class Engine:
    device_group_by = True                     # go(..., group_by=...) groups a device-resident result (pipeline.py)
    device_order_by = True                     # go(..., order_by=...) selects a device-resident result's top rows
    device_group_order = True                  # go(..., group_by=..., order_by=...) does both in HBM in one call
    device_yield = True                        # go_yield: `GO | YIELD ... [WHERE ...]` filtered / reduced in HBM
    device_set_op = True                       # go_set(left, right, op) runs both GOs and the set operator in HBM
    device_find_path = True                    # find_path(space, sentence) searches FIND SHORTEST PATH in HBM
    path_paths_max = 1 << 20                   # find_path: FIND ALL / NOLOOP PATH answers with more walks are refused ("find path: more than ... paths")
    device_fetch = True                        # fetch(space, spec) / go_fetch(space, go, spec) look keys up and gather in HBM
    device_lookup = True                       # lookup(space, spec) scans a tag's / an edge type's columns in HBM

    def __init__(self, device: int = 0, rank: int = 0, world: int = 1, nccl_id: Optional[bytes] = None,
                 exchange=None):
        """world > 1: one shard per rank over RCCL (nccl_id from unique_id() on rank 0), or over a host
        collective `exchange` (dist_exchange()) when the ranks share a GPU."""
        self.L = lib()
        self._uid = ctypes.create_string_buffer(nccl_id, 128) if nccl_id else None
        self._xchg = exchange                      # keep the ctypes callback alive with the context
        cfg = Config(device, rank, world, ctypes.cast(self._uid, ctypes.c_void_p) if self._uid else None,
                     ctypes.cast(exchange, ctypes.c_void_p) if exchange else None, None)
        h = ctypes.c_void_p()
        rc = self.L.ngx_open(ctypes.byref(cfg), ctypes.byref(h))
        if rc:
            raise EngineError(rc, "ngx_open failed (no HIP device or RCCL init failed)")
        self.h = h
        self.rank, self.world = rank, world
        self._parts: Dict[int, int] = {}                          # what catalog() hands the FETCH executors
        self._schemas: Dict[int, list] = {}

    def close(self):
        if getattr(self, "h", None):
            self.L.ngx_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, what: str):
        if rc:
            raise EngineError(rc, f"{what}: {self.L.ngx_last_error(self.h).decode()}")

    # ---- schema + data
    def add_space(self, space: int, num_parts: int):
        self._check(self.L.ngx_add_space(self.h, space, num_parts), "add_space")
        self._parts[space] = num_parts

    def add_schema(self, space, is_edge, sid, name, fields: Sequence[Tuple[str, int]], ver=0, ttl_col="", ttl_dur=0):
        names = (ctypes.c_char_p * max(1, len(fields)))(*[f[0].encode() for f in fields])
        types = (c_i32 * max(1, len(fields)))(*[f[1] for f in fields])
        self._check(self.L.ngx_add_schema(self.h, space, 1 if is_edge else 0, sid, name.encode(), ver, len(fields),
                                          names, types, ttl_col.encode(), ttl_dur), "add_schema")
        self._schemas.setdefault(space, []).append((bool(is_edge), sid, name, list(fields), ver))

    def catalog(self, space: int):
        """The space's fetch.Catalog (partition count, latest tag and edge schemas) from what add_space and
        add_schema were given: what the FETCH executors ask the schema manager."""
        from . import fetch
        from types import SimpleNamespace as NS
        return fetch.Catalog.of(self._parts[space], [NS(is_edge=e, sid=i, name=n, fields=f, ver=v)
                                                      for e, i, n, f, v in self._schemas.get(space, [])])

    def load_kv(self, space: int, keys, koff, vals, voff):
        keys, vals = np.ascontiguousarray(keys, dtype=np.uint8), np.ascontiguousarray(vals, dtype=np.uint8)
        koff, voff = np.ascontiguousarray(koff, dtype=np.uint64), np.ascontiguousarray(voff, dtype=np.uint64)
        b = KVBatchC(len(koff) - 1, keys.ctypes.data, koff.ctypes.data, vals.ctypes.data, voff.ctypes.data)
        self._check(self.L.ngx_load_kv(self.h, space, ctypes.byref(b)), "load_kv")

    def load_csr(self, space: int, vpart, vid, slots):
        """ngx_load_csr: this shard's vertex table (sorted by (part, vid)) and per slot (etype, off, dst,
        [column arrays of the latest schema's fields][, ranks]) as int64 / uint64 arrays (datagen.Csr.slots); without
        the fifth entry every edge has rank 0."""
        vpart = np.ascontiguousarray(vpart, dtype=np.int32)
        vid = np.ascontiguousarray(vid, dtype=np.int64)
        keep = [vpart, vid]
        cs = (CsrSlotC * max(1, len(slots)))()
        for k, slot in enumerate(slots):
            etype, off, dst, cols = slot[:4]
            off = np.ascontiguousarray(off, dtype=np.uint64)
            dst = np.ascontiguousarray(dst, dtype=np.int64)
            cols = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
            ptrs = (ctypes.c_void_p * max(1, len(cols)))(*[c.ctypes.data for c in cols])
            rank = np.ascontiguousarray(slot[4], dtype=np.int64) if len(slot) > 4 and slot[4] is not None else None
            keep += [off, dst, cols, ptrs, rank]
            cs[k] = CsrSlotC(int(etype), off.ctypes.data, dst.ctypes.data, rank.ctypes.data if rank is not None else None, len(cols),
                             ctypes.cast(ptrs, ctypes.c_void_p))
        sh = CsrShardC(len(vid), vpart.ctypes.data, vid.ctypes.data, len(slots), cs)
        self._check(self.L.ngx_load_csr(self.h, space, ctypes.byref(sh)), "load_csr")
        del keep

    def load_batch(self, space: int, batch):
        self.load_kv(space, *batch.arrays())

    def load_snapshot_rows(self, space: int, rows: bytes):
        """Stage a part's snapshot stream: encodeKV records (kvfmt.encode_kv), as SnapshotManagerImpl
        streams them (src/kvstore/SnapshotManagerImpl.cpp:15-53)."""
        buf = ctypes.create_string_buffer(bytes(rows), len(rows)) if rows else None
        self._check(self.L.ngx_load_snapshot_rows(self.h, space, buf, len(rows)), "load_snapshot_rows")

    def save_snapshot(self, space: int, path: str, tag: str = ""):
        self._check(self.L.ngx_save_snapshot(self.h, space, path.encode(), tag.encode()), "save_snapshot")

    def open_snapshot(self, space: int, path: str) -> str:
        """Load a device snapshot file saved by save_snapshot; returns its checkpoint tag."""
        tag = ctypes.create_string_buffer(64)
        self._check(self.L.ngx_open_snapshot(self.h, space, path.encode(), tag), "open_snapshot")
        return tag.value.decode()

    def commit(self, space: int):
        self._check(self.L.ngx_commit(self.h, space), "commit")

    def info(self, space: int) -> GraphInfo:
        gi = GraphInfo()
        self._check(self.L.ngx_graph_info_get(self.h, space, ctypes.byref(gi)), "graph_info")
        return gi

    # ---- GetNeighbors
    def get_neighbors(self, space, parts: Sequence[Tuple[int, Sequence[int]]], edge_types: Optional[Sequence[int]],
                      return_columns: Sequence[Tuple[int, int, str]], filter_bytes: bytes = b"",
                      max_edges_per_vertex: int = 2**31 - 1, now_sec: int = 0,
                      encode_rows: bool = False, decode: bool = True) -> NeighborsResult:
        """decode=False: counts and failed codes only (no Python cells; the bench's latency loop)."""
        pid = np.array([p for p, _ in parts], dtype=np.int32)
        nv = np.array([len(v) for _, v in parts], dtype=np.uint32)
        vids = np.array([x for _, v in parts for x in v], dtype=np.int64)
        et = np.array(list(edge_types or []), dtype=np.int32)
        cols = (PropDef * max(1, len(return_columns)))(*[PropDef(o, i, n.encode()) for o, i, n in return_columns])
        req = GnRequest(space, len(parts), pid.ctypes.data_as(P(c_i32)), nv.ctypes.data_as(P(c_u32)),
                        vids.ctypes.data_as(P(c_i64)), len(et), et.ctypes.data_as(P(c_i32)), filter_bytes,
                        len(filter_bytes), len(return_columns), cols, max_edges_per_vertex, now_sec,
                        1 if encode_rows else 0)
        out = P(GnResult)()
        rc = self.L.ngx_get_neighbors(self.h, ctypes.byref(req), ctypes.byref(out))
        try:
            r = out.contents
            if rc and rc not in (NGX_OK,) and r.nfailed == 0:
                raise EngineError(rc, self.L.ngx_last_error(self.h).decode())
            failed = [(r.failed_codes[2 * i], r.failed_codes[2 * i + 1]) for i in range(r.nfailed)]
            if not decode:
                return NeighborsResult(code=r.code, failed_codes=failed, total_edges=r.nedges, edge_vertex=None,
                                       edge_type=None, edge_dst=None, edge_cells=[], vertex_cells=[],
                                       vertex_has_tag=None, latency_in_us=r.latency_in_us)
            strings = ctypes.string_at(r.strings, r.strings_len) if r.strings_len else b""
            nc = r.ncols
            enc = {}
            if encode_rows:
                off = _arr(r.edge_props_off, r.nedges + 1, np.uint64)
                blob = ctypes.string_at(r.edge_props, int(off[-1])) if r.nedges and off[-1] else b""
                enc["edge_props"] = [blob[int(off[i]):int(off[i + 1])] for i in range(r.nedges)]
                es, vs = {}, {}
                for k in range(r.nschemas):
                    sd = r.schemas[k]
                    cols_ = [(sd.names[j].decode(), sd.types[j]) for j in range(sd.ncols)]
                    (es if sd.is_edge else vs)[sd.id] = cols_
                enc["edge_schema"], enc["vertex_schema"] = es, vs
                toff = _arr(r.tag_props_off, r.ntag_rows + 1, np.uint64)
                tblob = ctypes.string_at(r.tag_props, int(toff[-1])) if r.ntag_rows and toff[-1] else b""
                enc["tag_rows"] = [(int(r.tag_row_vertex[k]), int(r.tag_row_tag[k]), tblob[int(toff[k]):int(toff[k + 1])])
                                   for k in range(r.ntag_rows)]
            return NeighborsResult(
                code=r.code, failed_codes=failed, total_edges=r.nedges,
                edge_vertex=_arr(r.edge_vertex, r.nedges, np.uint32), edge_type=_arr(r.edge_type, r.nedges, np.int32),
                edge_dst=_arr(r.edge_dst, r.nedges, np.int64),
                edge_cells=_cells(r.edge_cells, r.nedges, nc, strings),
                vertex_cells=_cells(r.vertex_cells, r.nvertices, nc, strings),
                vertex_has_tag=_arr(r.vertex_has_tag, r.nvertices * nc, np.uint8),
                latency_in_us=r.latency_in_us, **enc)
        finally:
            self.L.ngx_gn_result_free(out)

    # ---- GO
    def go(self, space: int, s: Union[str, ngql.GoSentence], pushdown: bool = True, now_sec: int = 0,
           raise_on_error: bool = False, rows: bool = True, on_device: bool = False, fetch: bool = False,
           columnar: bool = False, digest_fn=None, arrays: bool = True, input=None,
           yield_only: bool = False, compact: bool = False, device_digest: bool = False,
           group_by: Optional[GroupBySpec] = None, order_by: Optional[OrderBySpec] = None,
           yield_by: Optional[YieldSpec] = None) -> GoResult:
        """Run one GO. rows=False skips decoding cells into Python tuples; on_device=True leaves the
        result rows in HBM (GoResult.nrows and the statistics only); with fetch=True the HBM arrays
        (src/dst/rank/type and the columnar YIELD columns) are copied back into the result.
        columnar=True asks for host_columnar results: no cells; with rows=True they are rebuilt here
        from the columns (ColumnValue typing by col_types) so they compare with the cell path.
        digest_fn(col_types, nrows, x_ptrs, len_ptrs, type_ptrs) is called on the host columns
        before the result is freed (tests: large-result comparison). FROM $-.col / $var.col reads
        `input' (a nebula_amd.pipeline.Interim; None: no input, no rows). yield_only (with on_device):
        only the YIELD columns are materialised; src / dst / rank arrays only where a column aliases them.
        device_digest (with on_device): GoResult.device_digest = (sum, xor, rows) of the row hashes, computed
        on the device (ngx_go_result_digest; oracle.row_digest restates it).
        compact (with on_device): integer result arrays at the widths of the stored columns they copy
        (ngx_go_plan.compact_results); fetch widens them back to int64 (GoResult.dev_widths keeps them).
        group_by: the GO runs with on_device and its rows are grouped in HBM (ngx_go_group_by) before the
        result is freed; GoResult.rows / col_types / nrows are then the group rows, device_ms the grouping's
        and group_device_ms too (go_device_ms keeps the traversal's). NGX_E_UNSUPPORTED comes back as a
        result with that code and the reason (the caller groups on the host), not as an exception.
        order_by: likewise, rows [offset, offset + count) of the result ordered by the spec's factors are
        selected in HBM (ngx_go_order_by); GoResult.rows / nrows are those rows in order, col_types the GO's,
        device_ms / order_device_ms the selection's, order_host_sort_ms the library's sort of the winners.
        group_by and order_by together: the group rows are ordered and cut in HBM too (ngx_go_group_order_by;
        the spec's factors name yield columns of group_by); rows / nrows / col_types describe the window of
        group rows, device_ms / group_device_ms / order_device_ms are the one call's time.
        yield_by: likewise, the `| YIELD ... [WHERE ...]` sentence behind the GO runs over its rows in HBM
        (ngx_go_yield, go_yield below)."""
        if group_by is not None or order_by is not None or yield_by is not None:
            on_device, columnar = True, False
        if isinstance(s, PreparedGo):                       # its own pushdown / result-placement flags
            plan, keep = s.plan, s
            on_device, columnar = bool(plan.result_on_device), bool(plan.host_columnar)
        else:
            if isinstance(s, str):
                s = ngql.parse_go(s)
            keep = self.prepare_go(space, s, pushdown=pushdown, now_sec=now_sec, on_device=on_device,
                                   columnar=columnar, yield_only=yield_only, input=input, compact=compact)
            plan = keep.plan
        out = P(GoResultC)()
        rc = self.L.ngx_go(self.h, ctypes.byref(plan), ctypes.byref(out))
        try:
            r = out.contents
            err = self.L.ngx_last_error(self.h).decode() if rc else ""
            if rc and (raise_on_error or rc in (E_DEVICE, E_UNSUPPORTED)):
                raise EngineError(rc, err)
            strings = ctypes.string_at(r.strings, r.strings_len) if r.strings_len else b""
            n = r.nrows
            if on_device:
                # pointer slices (one C loop each) rather than an element access per index: this path
                # runs once per bench step
                nh, nc = r.nhops, r.ncols
                xb = r.hop_exchange_bytes
                res = GoResult(ok=rc == 0, error=err, code=rc, col_types=r.col_types[:nc] if nc else [],
                               rows=[], nrows=n, host_prep_ms=r.host_prep_ms, host_tail_ms=r.host_tail_ms,
                               hop_frontier=r.hop_frontier[:nh] if nh else [],
                               hop_edges=r.hop_edges[:nh] if nh else [],
                               hop_next=r.hop_next[:nh] if nh else [],
                               hop_xchg=xb[:nh] if xb and nh else [],
                               device_ms=r.device_ms)
                if rc == 0 and r.dev_col_w:
                    # width 0: a constant column (value in dev_key_const / dev_col_const, no array)
                    res.dev_widths = (r.dev_key_w[:3], r.dev_col_w[:nc] if nc else [])
                    res.dev_consts = (r.dev_key_const[:3], r.dev_col_const[:nc] if nc and r.dev_col_const else [0] * nc)
                if group_by is not None and order_by is not None and rc == 0:
                    self._group_order_by(out, group_by, order_by, res)
                elif group_by is not None and rc == 0:
                    self._group_by(out, group_by, res)
                elif order_by is not None and rc == 0:
                    self._order_by(out, order_by, res)
                elif yield_by is not None and rc == 0:
                    self._yield(out, yield_by, res, rows=rows)
                if device_digest and rc == 0:
                    d3 = (c_u64 * 3)()
                    drc = self.L.ngx_go_result_digest(self.h, out, d3)
                    if drc:
                        raise EngineError(drc, self.L.ngx_last_error(self.h).decode())
                    res.device_digest = (int(d3[0]), int(d3[1]), int(d3[2]))
                if fetch and rc == 0:
                    kw = res.dev_widths[0] if res.dev_widths else [8, 8, 8]
                    cw = res.dev_widths[1] if res.dev_widths else [8] * r.ncols
                    kc, cc = res.dev_consts if res.dev_widths else ([0, 0, 0], [0] * r.ncols)

                    def key(ptr, k):
                        if kw[k] == 0:
                            return np.full(n, kc[k], np.int64)
                        return self._d2h_int(ptr, n, kw[k]) if ptr else None
                    res.src = key(r.dev_src, 0)
                    res.dst = key(r.dev_dst, 1)
                    res.rank = key(r.dev_rank, 2)
                    res.etype = (self._d2h(r.dev_type, n, np.int32) if r.dev_type
                                 else np.full(n, r.dev_type_const, np.int32))   # one OVER type: no column
                    cols = ctypes.cast(r.dev_cols, P(DevColumn)) if r.dev_cols else None
                    for c in range(r.ncols):
                        dc = cols[c]
                        res.dev_cols.append((np.full(n, cc[c], np.int64) if cw[c] == 0 else self._d2h_int(dc.x, n, cw[c]),
                                             self._d2h(dc.len, n, np.uint32) if dc.len else None,
                                             self._d2h(dc.type, n, np.uint8) if dc.type else None))
                return res
            if columnar:
                if not arrays:                             # delivery only (bench): no Python copies
                    return GoResult(ok=rc == 0, error=err, code=rc, col_types=[r.col_types[i] for i in range(r.ncols)],
                                    rows=[], nrows=r.nrows, hop_edges=[r.hop_edges[i] for i in range(r.nhops)],
                                    device_ms=r.device_ms, host_prep_ms=r.host_prep_ms, host_tail_ms=r.host_tail_ms)
                return self._columnar(r, rc, err, rows, digest_fn)
            res = GoResult(
                ok=rc == 0, error=err, code=rc, col_types=[r.col_types[i] for i in range(r.ncols)],
                rows=_cells(r.cells, n, r.ncols, strings) if rows else [],
                src=_arr(r.row_src, n, np.int64), dst=_arr(r.row_dst, n, np.int64),
                rank=_arr(r.row_rank, n, np.int64), etype=_arr(r.row_type, n, np.int32),
                hop_frontier=[r.hop_frontier[i] for i in range(r.nhops)],
                hop_edges=[r.hop_edges[i] for i in range(r.nhops)],
                hop_next=[r.hop_next[i] for i in range(r.nhops)],
                               hop_xchg=[r.hop_exchange_bytes[i] for i in range(r.nhops)] if r.hop_exchange_bytes else [],
                               device_ms=r.device_ms, nrows=n)
            return res
        finally:
            self.L.ngx_go_result_free(out)

    @staticmethod
    def _group_plan(spec: GroupBySpec):
        """(GroupPlanC, the arrays it points into)"""
        keys = (c_i32 * max(1, len(spec.key_cols)))(*spec.key_cols)
        ys = (AggColC * max(1, len(spec.yields)))()
        for i, (fn, col, konst) in enumerate(spec.yields):
            ys[i].fn, ys[i].col = AGG_FN[fn], col
            if col < 0:
                if isinstance(konst, float):
                    ys[i].konst.kind, ys[i].konst.v.d = _CELL_KIND["double"], konst
                elif isinstance(konst, int) and not isinstance(konst, bool):
                    ys[i].konst.kind, ys[i].konst.v.i = _CELL_KIND["int"], konst
                else:
                    ys[i].konst.kind = _CELL_KIND["str"]
        return GroupPlanC(len(spec.key_cols), keys, len(spec.yields), ys), (keys, ys)

    @staticmethod
    def _order_plan(spec: OrderBySpec):
        fs = (OrderFactorC * max(1, len(spec.factors)))()
        for i, (col, desc) in enumerate(spec.factors):
            fs[i].col, fs[i].desc = col, 1 if desc else 0
        return OrderPlanC(len(spec.factors), fs, spec.offset, spec.count), fs

    def _group_by(self, go_out, spec: GroupBySpec, res: GoResult):
        plan, _keep = self._group_plan(spec)
        gout = P(GroupResultC)()
        rc = self.L.ngx_go_group_by(self.h, go_out, ctypes.byref(plan), ctypes.byref(gout))
        try:
            res.go_device_ms, res.go_nrows = res.device_ms, res.nrows
            if rc:
                err = self.L.ngx_last_error(self.h).decode()
                if rc != E_UNSUPPORTED:
                    raise EngineError(rc, err)
                res.ok, res.code, res.error = False, rc, err
                return
            g = gout.contents
            strings = ctypes.string_at(g.strings, g.strings_len) if g.strings_len else b""
            res.rows = _cells(g.cells, g.ngroups, g.ncols, strings)
            res.col_types = g.col_types[:g.ncols] if g.ngroups else []
            res.nrows = g.ngroups
            res.device_ms = res.group_device_ms = g.device_ms
        finally:
            self.L.ngx_group_result_free(gout)

    def _order_by(self, go_out, spec: OrderBySpec, res: GoResult, group: Optional[GroupBySpec] = None):
        plan, _keep = self._order_plan(spec)
        oout = P(OrderResultC)()
        if group is not None:
            gplan, _gkeep = self._group_plan(group)
            rc = self.L.ngx_go_group_order_by(self.h, go_out, ctypes.byref(gplan), ctypes.byref(plan), ctypes.byref(oout))
        else:
            rc = self.L.ngx_go_order_by(self.h, go_out, ctypes.byref(plan), ctypes.byref(oout))
        try:
            res.go_device_ms, res.go_nrows = res.device_ms, res.nrows
            if rc:
                err = self.L.ngx_last_error(self.h).decode()
                if rc != E_UNSUPPORTED:
                    raise EngineError(rc, err)
                res.ok, res.code, res.error = False, rc, err
                return
            o = oout.contents
            strings = ctypes.string_at(o.strings, o.strings_len) if o.strings_len else b""
            res.rows = _cells(o.cells, o.nrows, o.ncols, strings)
            res.col_types = o.col_types[:o.ncols] if o.ncols else []
            res.nrows = o.nrows
            res.device_ms = res.order_device_ms = o.device_ms
            res.order_host_sort_ms = o.host_sort_ms
            if group is not None:
                res.group_device_ms, res.ngroups = o.device_ms, o.input_rows
                if not o.input_rows:
                    res.col_types = []
        finally:
            self.L.ngx_order_result_free(oout)

    def go_yield(self, space: int, s: Union[str, ngql.GoSentence], spec: YieldSpec, pushdown: bool = True,
                 now_sec: int = 0) -> GoResult:
        """`s | YIELD ... [WHERE ...]`: the GO runs with its result left in HBM and the YIELD sentence filters,
        projects or reduces it there (ngx_go_yield); only the kept rows' cells, or the one aggregate row, cross.
        GoResult.rows / nrows / col_types are the sentence's (rows in the GO's row order), device_ms /
        yield_device_ms its device time, kept_rows the rows WHERE kept, go_nrows / go_device_ms the traversal's.
        NGX_E_UNSUPPORTED ("yield: ...") comes back as a result with that code and the reason: the caller runs
        the host restatement (nebula_amd/yieldexec.py)."""
        return self.go(space, s, pushdown=pushdown, now_sec=now_sec, yield_only=True, compact=True, yield_by=spec)

    def _yield(self, go_out, spec: YieldSpec, res: GoResult, rows: bool = True):
        names = (ctypes.c_char_p * max(1, len(spec.input_names)))(*[n.encode() for n in spec.input_names])
        ys = (YieldColC * max(1, len(spec.yields)))()
        for i, (fn, expr) in enumerate(spec.yields):
            ys[i].fn, ys[i].expr, ys[i].expr_len = AGG_FN[fn], expr, len(expr)
        where = spec.where or b""
        plan = YieldPlanC(len(spec.input_names), names, where, len(where), len(spec.yields), ys)
        yout = P(YieldResultC)()
        rc = self.L.ngx_go_yield(self.h, go_out, ctypes.byref(plan), ctypes.byref(yout))
        try:
            res.go_device_ms, res.go_nrows = res.device_ms, res.nrows
            if rc:
                err = self.L.ngx_last_error(self.h).decode()
                if rc != E_UNSUPPORTED:
                    raise EngineError(rc, err)
                res.ok, res.code, res.error = False, rc, err
                return
            y = yout.contents
            strings = ctypes.string_at(y.strings, y.strings_len) if y.strings_len else b""
            if rows:
                res.rows = _cells(y.cells, y.nrows, y.ncols, strings)
            else:                                                 # one copy of the cells, no Python tuples
                raw = ctypes.string_at(ctypes.cast(y.cells, ctypes.c_void_p).value, y.nrows * y.ncols * 16) if y.nrows else b""
                res.yield_cells = np.frombuffer(raw, dtype=[("kind", "<i4"), ("len", "<i4"), ("v", "<i8")]).reshape(y.nrows, y.ncols)
            res.col_types = y.col_types[:y.ncols] if y.input_rows else []   # the first input row types them
            res.nrows, res.kept_rows = y.nrows, y.kept_rows
            res.device_ms = res.yield_device_ms = y.device_ms
        finally:
            self.L.ngx_yield_result_free(yout)

    def _group_order_by(self, go_out, group: GroupBySpec, order: OrderBySpec, res: GoResult):
        self._order_by(go_out, order, res, group=group)

    def go_set(self, space: int, left: Union[str, ngql.GoSentence], right: Union[str, ngql.GoSentence], op: str,
               pushdown: bool = True, now_sec: int = 0, compact: bool = True, rows: bool = True) -> GoResult:
        """`left <op> right` with op "UNION" (DISTINCT), "INTERSECT" or "MINUS": both GOs run with their results
        left in HBM and the set operator runs there too (ngx_go_set); only the output rows cross. GoResult.rows /
        nrows / col_types are the output's, device_ms the set operator's, go_nrows the two inputs' rows together.
        NGX_E_UNSUPPORTED of the set stage ("set op: ...") comes back as a result with that code and the reason
        (the caller runs the host path); a traversal's own refusal raises, as go() does. rows=False skips decoding
        the cells into Python tuples: GoResult.digests is then the cells' value words as an int64 array of shape
        (nrows, ncols) (integers, double bits, string offsets)."""
        keep = [self.prepare_go(space, s, pushdown=pushdown, now_sec=now_sec, on_device=True, yield_only=True,
                                compact=compact) for s in (left, right)]
        plan = SetPlanC(SET_OP[op])
        out = P(SetResultC)()
        rc = self.L.ngx_go_set(self.h, ctypes.byref(keep[0].plan), ctypes.byref(keep[1].plan), ctypes.byref(plan),
                               ctypes.byref(out))
        try:
            err = self.L.ngx_last_error(self.h).decode() if rc else ""
            if rc in (E_DEVICE, E_UNSUPPORTED) and not err.startswith("set op:"):
                raise EngineError(rc, err)
            if rc == E_DEVICE:
                raise EngineError(rc, err)
            o = out.contents
            res = GoResult(ok=rc == 0, error=err, code=rc, col_types=o.col_types[:o.ncols] if o.ncols else [], rows=[],
                           nrows=o.nrows, device_ms=o.device_ms, go_nrows=o.left_rows + o.right_rows)
            if rc == 0 and rows:
                strings = ctypes.string_at(o.strings, o.strings_len) if o.strings_len else b""
                res.rows = _cells(o.cells, o.nrows, o.ncols, strings)
            elif rc == 0:
                raw = ctypes.string_at(ctypes.cast(o.cells, ctypes.c_void_p).value, o.nrows * o.ncols * ctypes.sizeof(Cell)) \
                    if o.nrows and o.ncols else b""
                cell = np.dtype([("kind", "<i4"), ("len", "<i4"), ("v", "<i8")])
                res.digests = np.frombuffer(raw, dtype=cell)["v"].reshape(o.nrows, o.ncols).copy()
            return res
        finally:
            self.L.ngx_set_result_free(out)

    def _fetch_plan(self, space: int, spec: FetchSpec):
        """(FetchPlanC, the arrays it points into)"""
        tags = (c_i32 * max(1, len(spec.tags)))(*spec.tags)
        ys = (FetchYieldC * max(1, len(spec.yields)))()
        for i, (kind, tag, fld, key, col) in enumerate(spec.yields):
            ys[i].kind, ys[i].tag, ys[i].field, ys[i].key, ys[i].col = kind, tag, fld.encode(), key, col
        keys = [np.ascontiguousarray(k, dtype=np.int64) for k in (spec.keys or [])]
        ptr = [k.ctypes.data_as(P(c_i64)) for k in keys] + [None] * (3 - len(keys))
        if spec.kind == FETCH_EDGE and spec.key_cols[2] < 0:
            ptr[2] = None
        plan = FetchPlanC(space, spec.kind, len(spec.tags), tags, spec.edge_type, (c_i32 * 3)(*spec.key_cols),
                          len(keys[0]) if keys else 0, ptr[0], ptr[1], ptr[2], 1 if spec.distinct else 0,
                          1 if spec.keep_missing else 0, len(spec.yields), ys)
        return plan, (tags, ys, keys)

    def _fetch_result(self, rc: int, out, rows: bool) -> GoResult:
        err = self.L.ngx_last_error(self.h).decode() if rc else ""
        if rc == E_DEVICE:
            raise EngineError(rc, err)
        o = out.contents
        res = GoResult(ok=rc == 0, error=err, code=rc, col_types=o.col_types[:o.ncols] if o.ncols else [], rows=[],
                       nrows=o.nrows, device_ms=o.device_ms, go_nrows=o.input_rows, tags_seen=o.tags_seen)
        if rc == 0 and rows:
            strings = ctypes.string_at(o.strings, o.strings_len) if o.strings_len else b""
            res.rows = _cells(o.cells, o.nrows, o.ncols, strings)
        return res

    def fetch(self, space: int, spec: FetchSpec, result=None, rows: bool = True) -> GoResult:
        """FETCH PROP ON over keys in HBM (ngx_fetch): the keys are the spec's host arrays, or with `result` (a
        GoResultC of this engine's device-resident result, or an object with a .struct holding one) that result's
        columns. GoResult.rows / nrows / col_types are the output's (the key columns, then the yields, in key
        order), go_nrows the keys looked up, tags_seen the ON tags met, device_ms the call's. NGX_E_UNSUPPORTED
        ("fetch: ...") and prepare-time errors come back as a result with the code and text."""
        plan, _keep = self._fetch_plan(space, spec)
        out = P(FetchResultC)()
        r = None if result is None else ctypes.byref(getattr(result, "struct", result))
        rc = self.L.ngx_fetch(self.h, r, ctypes.byref(plan), ctypes.byref(out))
        try:
            return self._fetch_result(rc, out, rows)
        finally:
            self.L.ngx_fetch_result_free(out)

    def go_fetch(self, space: int, go: Union[str, ngql.GoSentence], spec: FetchSpec, pushdown: bool = True,
                 now_sec: int = 0, compact: bool = True, rows: bool = True) -> GoResult:
        """`GO ... | FETCH PROP ON ... $-.col ...` in one device call (ngx_go_fetch): the GO's rows stay in HBM and the
        FETCH reads its key and input columns there; only the output rows cross. A refusal of the fetch stage
        ("fetch: ...") comes back as a result with that code; the traversal's own refusal raises, as go() does."""
        keep = self.prepare_go(space, go, pushdown=pushdown, now_sec=now_sec, on_device=True, yield_only=True, compact=compact)
        plan, _keep = self._fetch_plan(space, spec)
        out = P(FetchResultC)()
        rc = self.L.ngx_go_fetch(self.h, ctypes.byref(keep.plan), ctypes.byref(plan), ctypes.byref(out))
        try:
            if rc in (E_DEVICE, E_UNSUPPORTED) and not self.L.ngx_last_error(self.h).decode().startswith("fetch:"):
                raise EngineError(rc, self.L.ngx_last_error(self.h).decode())
            return self._fetch_result(rc, out, rows)
        finally:
            self.L.ngx_fetch_result_free(out)

    def lookup(self, space: int, spec: LookupSpec, rows: bool = True) -> GoResult:
        """LOOKUP ON a tag / an edge type as one streaming pass over its columns in HBM (ngx_lookup). GoResult.rows /
        nrows / col_types are the output's (VertexID | SrcVID, DstVID, Ranking, then the yields, in storage order),
        go_nrows the rows scanned, device_ms the call's. NGX_E_UNSUPPORTED ("lookup: ...") and plan errors come back
        as a result with the code and text: no host path stands behind a refusal."""
        def conds(items):
            arr = (LookupCondC * max(1, len(items)))()
            for i, (fld, kind, op, lo, hi, bits, sb) in enumerate(items):
                arr[i].field, arr[i].kind, arr[i].op, arr[i].lo, arr[i].hi = fld.encode(), kind, op, lo, hi
                arr[i].bits, arr[i].str, arr[i].str_len = bits, sb, len(sb)
            return arr
        fields, terms = conds(spec.fields), conds(spec.terms)
        ys = (ctypes.c_char_p * max(1, len(spec.yields)))(*[y.encode() for y in spec.yields])
        plan = LookupPlanC(space, 1 if spec.is_edge else 0, spec.schema_id, len(spec.fields), fields, len(spec.terms),
                           terms, len(spec.yields), ys)
        out = P(LookupResultC)()
        rc = self.L.ngx_lookup(self.h, ctypes.byref(plan), ctypes.byref(out))
        try:
            err = self.L.ngx_last_error(self.h).decode() if rc else ""
            if rc == E_DEVICE:
                raise EngineError(rc, err)
            o = out.contents
            res = GoResult(ok=rc == 0, error=err, code=rc, col_types=o.col_types[:o.ncols] if o.ncols else [], rows=[],
                           nrows=o.nrows, device_ms=o.device_ms, go_nrows=o.scanned_rows, keep_bytes=o.keep_bytes)
            if rc == 0 and rows:
                strings = ctypes.string_at(o.strings, o.strings_len) if o.strings_len else b""
                res.rows = _cells(o.cells, o.nrows, o.ncols, strings)
            return res
        finally:
            self.L.ngx_lookup_result_free(out)

    def find_path(self, space: int, s: Union[str, ngql.FindPathSentence], from_vids: Optional[Sequence[int]] = None,
                  to_vids: Optional[Sequence[int]] = None, rows: bool = True) -> GoResult:
        """`FIND SHORTEST PATH ...` searched in HBM (ngx_find_path): the levels, the meets and the sweeps run on the
        device, only the path DAG's edges cross, and the paths are enumerated from them here (findpath.paths_from_dag).
        from_vids / to_vids: the vids of a sentence whose FROM / TO read `$-` or a variable (findpath.setup_vids).
        GoResult.rows are one ("path", text) cell each, in no fixed order; nrows their number; go_nrows the path-DAG
        edges, hop_frontier [levels expanded], path_found the found targets' bits, device_ms the call's.
        NGX_E_UNSUPPORTED with a text starting "find path:" comes back as a result with that code (the caller runs the host restatement); any other failure
        as a result with its code and text too. rows=False skips the enumeration (GoResult.dev_cols keeps the edge
        arrays src, dst, type, rank, mask).
        With flag find_path_all set, FIND ALL PATH and FIND NOLOOP PATH are answered too: the device returns the layered
        edge set (dev_cols gains a sixth array, each edge's layer), findpath.paths_from_layers enumerates the walks, and
        a sentence with more than path_paths_max ALL walks is refused like any other (counted here, after the call)."""
        from . import findpath
        if isinstance(s, str):
            s = ngql.parse_find_path(s)
        fv = list(s.from_vids if from_vids is None else from_vids)
        tv = list(s.to_vids if to_vids is None else to_vids)
        if (from_vids is None and s.from_type) or (to_vids is None and s.to_type):
            raise EngineError(E_BAD_ARGUMENT, "find_path: the sentence reads $- or a variable; pass from_vids / to_vids")
        keys = [a or n for n, a in s.over]
        if len(set(keys)) != len(keys):                           # prepareOver's `edge alias(...) was dup`: the host words it
            return GoResult(ok=False, error="find path: an edge alias listed twice", code=E_UNSUPPORTED, col_types=[], rows=[])
        fa, ta = np.array(fv, dtype=np.int64), np.array(tv, dtype=np.int64)
        names = (ctypes.c_char_p * max(1, len(s.over)))(*[n.encode() for n, _ in s.over])
        plan = PathPlanC(space, PATH_KIND[s.kind], len(fa), fa.ctypes.data_as(P(c_i64)), len(ta), ta.ctypes.data_as(P(c_i64)),
                         len(s.over), names, 1 if s.over_all else 0, s.direction, min(int(s.upto), 2 ** 32 - 1))
        out = P(PathResultC)()
        rc = self.L.ngx_find_path(self.h, ctypes.byref(plan), ctypes.byref(out))
        try:
            err = self.L.ngx_last_error(self.h).decode() if rc else ""
            if rc == E_DEVICE:
                raise EngineError(rc, err)
            o = out.contents
            res = GoResult(ok=rc == 0, error=err, code=rc, col_types=[], rows=[], device_ms=o.device_ms, go_nrows=o.nedges,
                           hop_frontier=[o.levels], path_found=int(o.found))
            if rc:
                return res
            m = o.nedges
            cols = (_arr(o.src, m, np.int64), _arr(o.dst, m, np.int64), _arr(o.type, m, np.int32), _arr(o.rank, m, np.int64),
                    _arr(o.mask, m, np.uint64))
            res.dev_cols = list(cols)
            layered = s.kind != "SHORTEST"
            if layered:
                res.dev_cols.append(_arr(o.layer, m, np.uint8))
            if rows:
                type_names = {o.edge_types[i]: o.edge_names[i].decode() for i in range(o.nedge_names)}
                if layered:
                    try:
                        texts = findpath.paths_from_layers(fv, tv, res.dev_cols[5], *cols, type_names, s.kind == "NOLOOP",
                                                           self.path_paths_max)
                    except findpath.FindPathRefusal as e:         # the walks are counted here: refused like the library's own
                        return GoResult(ok=False, error=str(e), code=E_UNSUPPORTED, col_types=[], rows=[], device_ms=o.device_ms,
                                        go_nrows=o.nedges, hop_frontier=[o.levels], path_found=int(o.found))
                else:
                    texts = findpath.paths_from_dag(fv, tv, *cols, type_names)
                res.rows = [(("path", t),) for t in texts]
                res.nrows = len(res.rows)
                res.col_types = [findpath.T_PATH] if res.rows else []
            return res
        finally:
            self.L.ngx_path_result_free(out)

    def go_batch(self, prepared: Sequence["PreparedGo"], digests: bool = False):
        """Run prepared GO plans back to back in one native call (ngx_go_batch): per query (code, result
        rows, edges scanned over all hops), plus with `digests` the device-resident result's digest
        (sum, xor, count as ngx_go_result_digest; zeros for a failed query)."""
        n = len(prepared)
        arr = (ctypes.POINTER(GoPlan) * max(n, 1))(*[ctypes.pointer(p.plan) for p in prepared])
        codes, rows, edges = (c_i32 * max(n, 1))(), (c_u64 * max(n, 1))(), (c_u64 * max(n, 1))()
        dg = (c_u64 * max(3 * n, 1))() if digests else None
        rc = self.L.ngx_go_batch(self.h, ctypes.cast(arr, ctypes.c_void_p), n, codes, rows, edges, dg)
        if rc != 0 and all(codes[i] == 0 for i in range(n)):
            raise EngineError(rc, "go_batch: " + self.L.ngx_last_error(self.h).decode())
        out = [(int(codes[i]), int(rows[i]), int(edges[i])) for i in range(n)]
        if digests:
            out = [o + ((int(dg[3 * i]), int(dg[3 * i + 1]), int(dg[3 * i + 2])),) for i, o in enumerate(out)]
        return out

    def prepare_go(self, space: int, s, pushdown: bool = True, now_sec: int = 0, on_device: bool = False,
                   columnar: bool = False, yield_only: bool = False, input=None, compact: bool = False) -> PreparedGo:
        """Encode a GO sentence (expressions in Expression::encode bytes, vids as int64) into the C plan
        once; go() accepts the result in place of the sentence (the bench's timed loop)."""
        if isinstance(s, str):
            s = ngql.parse_go(s)
        starts = np.array(s.vids, dtype=np.int64)
        names = (ctypes.c_char_p * max(1, len(s.over)))(*[n.encode() for n, _ in s.over])
        aliases = (ctypes.c_char_p * max(1, len(s.over)))(*[(a or "").encode() for _, a in s.over])
        where = s.where.encode() if s.where is not None else b""
        yb = [y.expr.encode() for y in s.yields]
        yarr = (ctypes.c_char_p * max(1, len(yb)))(*yb)
        ylen = (c_u32 * max(1, len(yb)))(*[len(y) for y in yb])
        plan = GoPlan(space, s.record_from, s.record_to, len(starts), starts.ctypes.data_as(P(c_i64)), len(s.over),
                      names, aliases, 1 if s.over_all else 0, s.direction, where if where else None, len(where),
                      len(yb), yarr, ylen, 1 if s.distinct else 0, 1 if pushdown else 0, now_sec,
                      1 if on_device else 0, 1 if columnar else 0)
        plan.yield_only = 1 if yield_only else 0
        plan.compact_results = 1 if compact else 0
        keep = [starts, names, aliases, where, yb, yarr, ylen]
        if s.from_type:
            from .pipeline import Interim
            inp = _input_arrays(input if input is not None else Interim([]))
            names_a, types_a, cells_a, strings_a, nc, nr = inp
            fcol = s.from_col.encode()
            fvar = s.from_var.encode() if s.from_type == 2 else None
            plan.input_vid_col = fcol
            plan.input_var = fvar
            plan.input_ncols, plan.input_nrows = nc, nr
            plan.input_names, plan.input_types, plan.input_cells = names_a, types_a, cells_a
            plan.input_strings = strings_a
            keep += [inp, fcol, fvar]
        return PreparedGo(plan, keep)

    def _columnar(self, r, rc, err, rows, digest_fn=None):
        n = r.nrows
        types = [r.col_types[i] for i in range(r.ncols)]
        res = GoResult(ok=rc == 0, error=err, code=rc, col_types=types, rows=[], nrows=n,
                       hop_frontier=[r.hop_frontier[i] for i in range(r.nhops)],
                       hop_edges=[r.hop_edges[i] for i in range(r.nhops)],
                       hop_next=[r.hop_next[i] for i in range(r.nhops)],
                               hop_xchg=[r.hop_exchange_bytes[i] for i in range(r.nhops)] if r.hop_exchange_bytes else [],
                               device_ms=r.device_ms)
        if rc != 0:
            return res
        res.src, res.dst, res.rank = _arr(r.row_src, n, np.int64), _arr(r.row_dst, n, np.int64), \
            _arr(r.row_rank, n, np.int64)
        res.etype = _arr(r.row_type, n, np.int32) if r.row_type else np.full(n, r.dev_type_const, np.int32)
        cols = ctypes.cast(r.host_cols, P(DevColumn)) if r.host_cols else None
        if digest_fn is not None:
            res.digests = digest_fn(types, n, [cols[c].x for c in range(r.ncols)],
                                    [cols[c].len for c in range(r.ncols)], [cols[c].type for c in range(r.ncols)])
            if not rows:
                return res
        for c in range(r.ncols):
            dc = cols[c]
            x = _arr(ctypes.cast(dc.x, P(c_i64)), n, np.int64)
            ln = _arr(ctypes.cast(dc.len, P(c_u32)), n, np.uint32) if dc.len else None
            t = _arr(ctypes.cast(dc.type, P(ctypes.c_uint8)), n, np.uint8) if dc.type else None
            res.dev_cols.append((x, ln, t))
        if rows:
            static = {1: 3, 2: 1, 3: 1, 21: 1, 4: 2, 5: 2, 6: 4}         # SupportedType -> V_* of its rows
            kinds = {1: "bool", 2: "int", 3: "id", 21: "timestamp", 4: "float", 5: "double", 6: "str"}
            out = []
            for i in range(n):
                row = []
                for c, (x, ln, t) in enumerate(res.dev_cols):
                    vt = int(t[i]) if t is not None else static.get(types[c], 0)
                    v = int(x[i])
                    if vt == 4:
                        row.append(("str", ctypes.string_at(v, int(ln[i])).decode("utf-8", "surrogateescape")
                                    if ln[i] else ""))
                    elif vt == 2:
                        row.append((kinds.get(types[c], "double"), float(np.int64(v).view(np.float64))))
                    elif vt == 3:
                        row.append(("bool", bool(v)) if types[c] == 1 else ("empty", bool(v)))
                    elif vt == 1:
                        row.append((kinds.get(types[c], "int"), v))
                    else:
                        row.append(("empty", None))
                out.append(tuple(row))
            res.rows = out
        return res

    def _d2h(self, ptr, n, dtype):
        out = np.zeros(n, dtype=dtype)
        if n and ptr:
            self._check(self.L.ngx_device_to_host(self.h, out.ctypes.data, ptr, out.nbytes), "device_to_host")
        return out

    def _d2h_int(self, ptr, n, width):
        """A device array of n signed integers at `width` bytes each, widened to int64."""
        dt = {1: np.int8, 2: np.int16, 4: np.int32}.get(int(width), np.int64)
        return self._d2h(ptr, n, dt).astype(np.int64, copy=False)

    # ---- flags
    def set_flag(self, name: str, value: int):
        self._check(self.L.ngx_set_flag(self.h, name.encode(), int(value)), "set_flag")

    def get_flag(self, name: str) -> int:
        v = c_i64()
        self._check(self.L.ngx_get_flag(self.h, name.encode(), ctypes.byref(v)), "get_flag")
        return v.value

    def jit_note(self) -> str:
        return self.L.ngx_jit_note(self.h).decode()

    # ---- measurement
    def set_profiling(self, on: bool):
        self._check(self.L.ngx_set_profiling(self.h, 1 if on else 0), "set_profiling")

    def stats(self) -> Dict[str, int]:
        """Service counters (storage_get_bound_qps / _error_qps / _latency_us_*), as ngx_stats names them."""
        p = P(Stat)()
        n = c_i32()
        self._check(self.L.ngx_stats(self.h, ctypes.byref(p), ctypes.byref(n)), "stats")
        return {p[i].name.decode(): p[i].value for i in range(n.value)}

    def kernel_stats(self) -> Dict[str, Tuple[int, float, int]]:
        p = P(KernelStat)()
        n = c_i32()
        self._check(self.L.ngx_kernel_stats(self.h, ctypes.byref(p), ctypes.byref(n)), "kernel_stats")
        return {p[i].name.decode(): (p[i].launches, p[i].total_ms, p[i].algo_bytes) for i in range(n.value)}


def build_info() -> dict:
    """ngx_build_info() parsed, plus whether its source digest matches the sources in this tree."""
    import hashlib
    import glob
    raw = lib().ngx_build_info().decode()
    info = dict(kv.split("=", 1) for kv in raw.replace(" built=", " built=").split(" ") if "=" in kv)
    csrc = os.path.join(HERE, "csrc")
    srcs = sorted(glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.h")) +
                  glob.glob(os.path.join(csrc, "*.hip")) +
                  [os.path.join(csrc, "../../include/nebula_gn.h"), os.path.join(csrc, "exports.map"),
                   os.path.join(csrc, "Makefile")], key=lambda p: os.path.relpath(p, csrc))
    h = hashlib.sha256()
    for p in srcs:
        with open(p, "rb") as f:
            h.update(f.read())
    info["tree_sha"] = h.hexdigest()[:16]
    info["matches_tree"] = info.get("src_sha") == info["tree_sha"]
    info["raw"] = raw
    return info


def hash_string(s: str) -> int:
    b = s.encode()
    return lib().ngx_hash_string(b, len(b))
