// `| YIELD <columns> [WHERE <expr>]` over a device-resident GO result (ngx_go_yield): the host driver of yield.hip.
#include "engine_ctx.h"

namespace {

using YieldResultHolder = CellResult<ngx_yield_result>;

bool yIntLike(int32_t t) { return t == NGX_T_INT || t == NGX_T_VID || t == NGX_T_TIMESTAMP; }

int32_t vtOfType(int32_t t) {
    switch (t) {
        case NGX_T_BOOL: return V_BOOL;
        case NGX_T_INT: case NGX_T_VID: case NGX_T_TIMESTAMP: return V_INT;
        case NGX_T_DOUBLE: return V_DBL;
        case NGX_T_STRING: return V_STR;
        default: return V_ERR;
    }
}

void inputProps(const ExprNode& n, std::vector<std::string>& out) {
    if (n.kind == K_INPUT_PROP || n.kind == K_VAR_PROP) out.push_back(n.prop);
    for (const auto& k : n.kids) inputProps(*k, out);
}

// the column type the reference's output schema gives an expression that is no bare input column
// (calculateExprType; UNKNOWN: the type of its value on the first input row, Collector::getSchema)
int32_t exprColType(const ExprNode& n, uint32_t vt) {
    if (n.kind == K_CAST) {
        static const int32_t m[] = {NGX_T_INT, NGX_T_STRING, NGX_T_DOUBLE, NGX_T_BOOL, NGX_T_TIMESTAMP};
        if (n.op < 5) return m[n.op];
    }
    if (n.kind == K_REL || n.kind == K_LOGIC) return NGX_T_BOOL;
    return vt == V_INT ? NGX_T_INT : vt == V_DBL ? NGX_T_DOUBLE : vt == V_BOOL ? NGX_T_BOOL : NGX_T_STRING;
}

// how an aggregate row's cell is made of the state words
enum { kFinState = 0, kFinOrdered, kFinAvgInt, kFinAvgF64, kFinConst, kFinLast };
struct Final {
    int32_t kind = NGX_CELL_INT, src = kFinConst, slot = 0;
    int64_t konst = 0;
};

const char* const kRowFailed = "yield: an expression failed on a row";

// Every refusal is decided before a row is returned: the plan's own before the first launch; a failed or retyped
// evaluation after the sweep that met it, when the call answers with the refusal and no rows.
int32_t yieldOp(ngx_ctx* c, const ngx_go_result* r, const ngx_yield_plan* p, YieldResultHolder& R) {
    if (r->code != NGX_OK || (r->nrows && r->ncols && !r->dev_cols)) return fail(c, NGX_E_BAD_ARGUMENT, "yield: not a device-resident result");
    if (c->world > 1) return fail(c, NGX_E_UNSUPPORTED, "yield: world > 1 needs the shards' rows in one order and mergeable states");
    if (p->nyields < 1 || !p->yields || p->ncols_in != r->ncols || (p->ncols_in && !p->input_names) || (p->where_len && !p->where))
        return fail(c, NGX_E_BAD_ARGUMENT, "yield: no yield columns, or the input names are not the result's");
    if (p->nyields > kYieldMax) return fail(c, NGX_E_UNSUPPORTED, "yield: more than 64 yields");
    const uint64_t n = r->nrows;
    if (n >= (1ULL << 32)) return fail(c, NGX_E_UNSUPPORTED, "yield: 2^32 rows or more");
    const int32_t ny = p->nyields;

    std::map<std::string, int32_t> colOfName;
    for (int32_t i = 0; i < p->ncols_in; i++) {
        if (!p->input_names[i] || !colOfName.emplace(p->input_names[i], i).second)
            return fail(c, NGX_E_UNSUPPORTED, "yield: input column names are not unique");
    }
    // a column some expression reads, or a bare yield copies
    std::vector<uint8_t> readCol(std::max<int32_t>(r->ncols, 1), 0);
    auto useProps = [&](const ExprNode& e) -> int32_t {
        std::vector<std::string> props;
        inputProps(e, props);
        for (const std::string& name : props) {
            auto it = colOfName.find(name);
            if (it == colOfName.end()) return fail(c, NGX_E_UNSUPPORTED, "yield: column `" + name + "' is not in the input");
            const int32_t y = it->second, t = r->col_types[y];
            if (t == 0 || (n && r->dev_cols[y].type)) return fail(c, NGX_E_UNSUPPORTED, "yield: UNKNOWN-typed column (per-row value types)");
            if (t == NGX_T_FLOAT) return fail(c, NGX_E_UNSUPPORTED, "yield: FLOAT column");
            if (vtOfType(t) == V_ERR) return fail(c, NGX_E_UNSUPPORTED, "yield: a column of an unknown type");
            readCol[y] = 1;
        }
        return NGX_OK;
    };

    // ---- the plan: expressions decoded, typed and compiled
    Space noSpace;                                                // the expressions name no tag or edge
    GraphdCtx gctx;
    gctx.sp = &noSpace;
    gctx.deviceLibm = c->deviceLibm;
    gctx.inputCols = &colOfName;
    std::vector<Insn> code;
    std::string pool;
    std::string err;
    auto compile = [&](const ExprNode& e, int32_t& off, uint64_t& poolOff) -> int32_t {
        Program prog;
        if (int32_t rc = compileGraphd(e, gctx, prog, err)) {
            (void)rc;
            return fail(c, NGX_E_UNSUPPORTED, "yield: " + err);
        }
        off = static_cast<int32_t>(code.size());
        poolOff = pool.size();
        code.insert(code.end(), prog.code.begin(), prog.code.end());
        pool += prog.pool;
        return NGX_OK;
    };
    int32_t whereOff = -1;
    uint64_t wherePool = 0;
    if (p->where_len) {
        auto w = decodeExpr(p->where, p->where_len, err);
        if (!w) return fail(c, NGX_E_BAD_ARGUMENT, "yield: WHERE: " + err);
        if (int32_t rc = useProps(*w)) return rc;
        if (int32_t rc = compile(*w, whereOff, wherePool)) return rc;
    }
    bool aggregate = false;
    for (int32_t y = 0; y < ny; y++) {
        const int32_t fn = p->yields[y].fn;
        if (fn == NGX_AGG_COUNT_DISTINCT) return fail(c, NGX_E_UNSUPPORTED, "yield: COUNT_DISTINCT keeps every distinct value");
        if (fn == NGX_AGG_STD) return fail(c, NGX_E_UNSUPPORTED, "yield: STD keeps every value");
        if (fn < NGX_AGG_GROUP || fn > NGX_AGG_BIT_XOR) return fail(c, NGX_E_BAD_ARGUMENT, "yield: unknown function");
        aggregate |= fn != NGX_AGG_GROUP;
    }
    std::vector<std::unique_ptr<ExprNode>> exprs(ny);
    std::vector<YieldItem> items(ny);
    for (int32_t y = 0; y < ny; y++) {
        const ngx_yield_col& yc = p->yields[y];
        if (!yc.expr || !yc.expr_len) return fail(c, NGX_E_BAD_ARGUMENT, "yield: a yield column without expression");
        exprs[y] = decodeExpr(yc.expr, yc.expr_len, err);
        if (!exprs[y]) return fail(c, NGX_E_BAD_ARGUMENT, "yield: " + err);
        const ExprNode& e = *exprs[y];
        YieldItem& it = items[y];
        it = YieldItem{};
        if (int32_t rc = useProps(e)) return rc;
        if (e.kind == K_INPUT_PROP || e.kind == K_VAR_PROP) {
            if (aggregate && yc.fn == NGX_AGG_GROUP) return fail(c, NGX_E_UNSUPPORTED, "yield: an input column without function beside an aggregate");
            it.mode = kYieldCol;
            it.a = colOfName[e.prop];
            it.cell = r->col_types[it.a];                         // NGX_CELL_* numbers its kinds as NGX_T_*
            it.vt = vtOfType(it.cell);
        } else if (yc.fn == NGX_AGG_COUNT && e.kind == K_PRIMARY) {
            it.mode = kYieldNone;                                 // COUNT(*), COUNT(1): nothing to evaluate
        } else {
            it.mode = kYieldEval;
            if (int32_t rc = compile(e, it.a, it.poolOff)) return rc;
        }
    }

    R.r.ncols = ny;
    R.r.input_rows = n;
    R.colTypes.assign(ny, 0);
    R.r.col_types = R.colTypes.data();
    if (n == 0) {                                                 // empty inputs: no rows, nothing to launch
        c->yieldDevice++;
        return NGX_OK;
    }

    // ---- descriptors: columns | items | slots | probes | error words
    std::vector<DResultCol> cols(r->ncols);
    for (int32_t y = 0; y < r->ncols; y++) {
        DResultCol& dc = cols[y];
        dc = DResultCol{};
        if (!readCol[y]) continue;
        const int32_t t = r->col_types[y];
        dc.vt = vtOfType(t);
        dc.w = t == NGX_T_STRING || t == NGX_T_DOUBLE ? 8 : r->dev_col_w ? r->dev_col_w[y] : 8;
        dc.konst = r->dev_col_const ? r->dev_col_const[y] : 0;
        dc.x = dc.w ? r->dev_cols[y].x : nullptr;
        dc.len = r->dev_cols[y].len;
        if (dc.w && !dc.x) return fail(c, NGX_E_BAD_ARGUMENT, "yield: column without values");
        if (dc.w != 0 && dc.w != 1 && dc.w != 2 && dc.w != 4 && dc.w != 8) return fail(c, NGX_E_BAD_ARGUMENT, "yield: column width");
        if (t == NGX_T_STRING && !dc.len) return fail(c, NGX_E_BAD_ARGUMENT, "yield: string column without lengths");
    }
    resultEvents(c);
    HIP_OK(hipEventRecord(c->gbEv[0], c->stream));
    constexpr size_t kMaxSlots = 2 * kYieldMax;
    const size_t colBytes = (cols.size() * sizeof(DResultCol) + 15) / 16 * 16;
    const size_t descBytes = colBytes + ny * sizeof(YieldItem) + kMaxSlots * sizeof(YieldSlot) + ny * sizeof(YieldProbe) + 16;
    char* desc = c->yDesc.get<char>(descBytes);
    DResultCol* colsDev = reinterpret_cast<DResultCol*>(desc);
    YieldItem* itemsDev = reinterpret_cast<YieldItem*>(desc + colBytes);
    YieldSlot* slotsDev = reinterpret_cast<YieldSlot*>(itemsDev + ny);
    YieldProbe* probeDev = reinterpret_cast<YieldProbe*>(slotsDev + kMaxSlots);
    uint32_t* errDev = reinterpret_cast<uint32_t*>(probeDev + ny);
    code.push_back(Insn{});                                       // OP_END: never an empty upload
    Insn* codeDev = c->yCode.get<Insn>(code.size());
    char* poolDev = c->yPool.get<char>(std::max<size_t>(pool.size(), 1));
    if (!cols.empty()) HIP_OK(hipMemcpyAsync(colsDev, cols.data(), cols.size() * sizeof(DResultCol), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(codeDev, code.data(), code.size() * sizeof(Insn), hipMemcpyHostToDevice, c->stream));
    if (!pool.empty()) HIP_OK(hipMemcpyAsync(poolDev, pool.data(), pool.size(), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(errDev, 0, 16, c->stream));
    auto uploadItems = [&] {
        HIP_OK(hipMemcpyAsync(itemsDev, items.data(), ny * sizeof(YieldItem), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));                  // the descriptors are pageable: copied before they go
    };
    uploadItems();

    YieldArgs a{};
    a.n = n;
    a.cols = colsDev;
    a.code = codeDev;
    a.pool = poolDev;
    a.whereOff = whereOff;
    a.wherePool = wherePool;
    a.ny = ny;
    a.items = itemsDev;
    a.slots = slotsDev;
    a.err = errDev;
    a.gridMax = c->yieldGridMax;

    // the error words after the work enqueued so far; a set one is the call's refusal
    uint32_t errs[2] = {0, 0};
    auto checkErrs = [&]() -> int32_t {
        HIP_OK(hipMemcpyAsync(errs, errDev, sizeof errs, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        if (errs[1]) return fail(c, NGX_E_UNSUPPORTED, "yield: an expression needs a host-only construct");
        if (errs[0]) return fail(c, NGX_E_UNSUPPORTED, kRowFailed);
        return NGX_OK;
    };
    std::vector<YieldProbe> probe(ny);
    auto probeRow = [&](uint64_t row) {
        if (launchYieldProbe(a, row, probeDev, c->stream)) throw Error{NGX_E_DEVICE, "yield probe"};
        HIP_OK(hipMemcpyAsync(probe.data(), probeDev, ny * sizeof(YieldProbe), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    };

    // ---- the first input row types the columns (getOutputSchema)
    std::vector<int32_t> typeOf(ny, 0);
    bool anyEval = false;
    for (const YieldItem& it : items) anyEval |= it.mode == kYieldEval;
    if (anyEval) probeRow(0);
    for (int32_t y = 0; y < ny; y++) {
        YieldItem& it = items[y];
        if (it.mode == kYieldCol) { typeOf[y] = it.cell; continue; }
        if (it.mode == kYieldNone) { typeOf[y] = NGX_T_STRING; continue; }
        if (probe[y].vt == V_ERR) {
            if (int32_t rc = checkErrs()) return rc;
            return fail(c, NGX_E_UNSUPPORTED, kRowFailed);
        }
        if (probe[y].vt == V_STR) return fail(c, NGX_E_UNSUPPORTED, "yield: an expression whose value is a string");
        it.vt = static_cast<int32_t>(probe[y].vt);
        typeOf[y] = exprColType(*exprs[y], probe[y].vt);
        if (vtOfType(typeOf[y]) != it.vt) return fail(c, NGX_E_UNSUPPORTED, "yield: a value that is not of its column's type");
        it.cell = typeOf[y];
    }
    if (int32_t rc = checkErrs()) return rc;

    // ---- the aggregates' state words
    std::vector<YieldSlot> slots;
    std::vector<Final> fin(ny);
    if (aggregate) {
        auto slot = [&](int32_t op, int32_t src, int32_t y) {
            slots.push_back(YieldSlot{op, src, y, 0});
            return static_cast<int32_t>(slots.size() - 1);
        };
        slot(kGroupAdd, kYieldSrcOne, -1);                        // [0] the kept rows
        slot(kGroupMax, kYieldSrcRow, -1);                        // [1] the last kept row + 1
        for (int32_t y = 0; y < ny; y++) {
            const int32_t fn = p->yields[y].fn, t = typeOf[y];
            Final& f = fin[y];
            if (t == NGX_T_TIMESTAMP)                             // toColumnValue is asked for ColumnValue type 21
                return fail(c, NGX_E_UNSUPPORTED, "yield: a TIMESTAMP value beside an aggregate (the reference fails it: Wrong Type: 21)");
            switch (fn) {
                case NGX_AGG_GROUP:
                    f.kind = t, f.src = kFinLast;
                    break;
                case NGX_AGG_COUNT:
                    f.kind = NGX_CELL_INT, f.src = kFinState, f.slot = slot(kGroupAdd, kYieldSrcOne, y);
                    break;
                case NGX_AGG_SUM:
                    if (yIntLike(t)) f.kind = t, f.src = kFinState, f.slot = slot(kGroupAdd, kYieldSrcValue, y);
                    else if (t == NGX_T_DOUBLE) f.kind = NGX_CELL_DOUBLE, f.src = kFinState, f.slot = slot(kGroupAddF64, kYieldSrcValue, y);
                    else slot(kGroupAdd, kYieldSrcOne, y);        // Sum ignores values it cannot add; they are still evaluated
                    break;
                case NGX_AGG_AVG:
                    if (t == NGX_T_VID) return fail(c, NGX_E_UNSUPPORTED, "yield: AVG of a VID value (the reference reads the sum as a double)");
                    f.kind = NGX_CELL_DOUBLE;
                    if (t == NGX_T_INT) f.src = kFinAvgInt, f.slot = slot(kGroupAdd, kYieldSrcValue, y);
                    else if (t == NGX_T_DOUBLE) f.src = kFinAvgF64, f.slot = slot(kGroupAddF64, kYieldSrcValue, y);
                    else f.src = kFinAvgInt, f.slot = -1, slot(kGroupAdd, kYieldSrcOne, y);       // 0 / count
                    break;
                case NGX_AGG_MAX:
                case NGX_AGG_MIN: {
                    const int32_t op = fn == NGX_AGG_MAX ? kGroupMax : kGroupMin;
                    if (yIntLike(t)) f.kind = t, f.src = kFinState, f.slot = slot(op, kYieldSrcValue, y);
                    else if (t == NGX_T_DOUBLE) f.kind = NGX_CELL_DOUBLE, f.src = kFinOrdered, f.slot = slot(op, kYieldSrcOrdered, y);
                    else return fail(c, NGX_E_UNSUPPORTED, "yield: MAX / MIN of a BOOL or STRING value");
                    break;
                }
                default:                                          // BIT_*: integers only, anything else is ignored
                    if (t == NGX_T_INT)
                        f.kind = NGX_CELL_INT, f.src = kFinState,
                        f.slot = slot(fn == NGX_AGG_BIT_AND ? kGroupAnd : fn == NGX_AGG_BIT_OR ? kGroupOr : kGroupXor, kYieldSrcValue, y);
                    else slot(kGroupAdd, kYieldSrcOne, y);
                    break;
            }
        }
        if (slots.size() > kMaxSlots) return fail(c, NGX_E_UNSUPPORTED, "yield: more than 128 state words");
        HIP_OK(hipMemcpyAsync(slotsDev, slots.data(), slots.size() * sizeof(YieldSlot), hipMemcpyHostToDevice, c->stream));
    }
    a.nslots = static_cast<int32_t>(slots.size());
    uploadItems();                                                // with the value types of the first row

    // ---- keep
    const uint64_t chunks = (n + 255) / 256;
    uint64_t rowBytes = 0;
    for (const DResultCol& dc : cols) rowBytes += static_cast<uint64_t>(dc.w);
    if (whereOff >= 0) {
        a.keepBits = c->yKeep.get<uint64_t>((n + 63) / 64);
        a.chunkCount = c->yCount.get<uint64_t>(chunks + 1);
        c->timed("yield_keep", n * rowBytes + n / 8, [&] {
            if (launchYieldKeep(a, c->stream)) throw Error{NGX_E_DEVICE, "yield keep"};
        });
    }

    if (aggregate) {
        a.state = c->yState.get<uint64_t>(kMaxSlots);
        c->timed("yield_agg", n * rowBytes + n / 8, [&] {
            if (launchYieldAgg(a, c->stream)) throw Error{NGX_E_DEVICE, "yield aggregate"};
        });
        std::vector<uint64_t> state(slots.size());
        HIP_OK(hipMemcpyAsync(state.data(), a.state, state.size() * 8, hipMemcpyDeviceToHost, c->stream));
        if (int32_t rc = checkErrs()) return rc;
        const uint64_t kept = state[0];
        if (kept > n || (kept && (static_cast<int64_t>(state[1]) < 1 || state[1] > n))) throw Error{NGX_E_DEVICE, "yield: inconsistent counts"};
        if (!kept) std::fill(state.begin(), state.end(), 0);       // a function nothing was applied to: 0 (BIT_AND too)
        bool last = false;
        for (int32_t y = 0; y < ny; y++) {
            const int32_t fn = p->yields[y].fn;
            if (!kept && (fn == NGX_AGG_GROUP || fn == NGX_AGG_MAX || fn == NGX_AGG_MIN))
                return fail(c, NGX_E_UNSUPPORTED, "yield: no row kept under MAX / MIN / a yield without function (the reference fails it: Not Support: 0)");
            last |= fin[y].src == kFinLast && items[y].mode == kYieldEval;
        }
        if (last) {
            probeRow(state[1] - 1);
            for (int32_t y = 0; y < ny; y++)
                if (fin[y].src == kFinLast && static_cast<int32_t>(probe[y].vt) != items[y].vt) return fail(c, NGX_E_UNSUPPORTED, kRowFailed);
        }
        HIP_OK(hipEventRecord(c->gbEv[1], c->stream));
        R.cells.assign(ny, ngx_cell{});
        for (int32_t y = 0; y < ny; y++) {
            const Final& f = fin[y];
            ngx_cell& cell = R.cells[y];
            cell.kind = f.kind;
            const uint64_t w = f.src == kFinConst || f.slot < 0 ? 0 : state[f.slot];
            double d;
            switch (f.src) {
                case kFinState: cell.v.i = static_cast<int64_t>(w); break;
                case kFinOrdered: {
                    const int64_t k = static_cast<int64_t>(w);
                    cell.v.i = k ^ ((k >> 63) & 0x7FFFFFFFFFFFFFFFLL);
                    break;
                }
                case kFinAvgInt: cell.v.d = static_cast<double>(static_cast<int64_t>(w)) / static_cast<double>(kept); break;
                case kFinAvgF64: std::memcpy(&d, &w, 8); cell.v.d = d / static_cast<double>(kept); break;
                case kFinLast: cell.v.i = probe[y].x; break;
                default: cell.v.i = f.konst; break;
            }
            if (!kept && p->yields[y].fn == NGX_AGG_SUM) cell.kind = NGX_CELL_INT, cell.v.i = 0;   // Sum's result with nothing added
            R.colTypes[y] = cell.kind;
        }
        HIP_OK(hipStreamSynchronize(c->stream));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, c->gbEv[0], c->gbEv[1]));
        c->collectTimings();
        R.r.device_ms = ms;
        R.r.cells = R.cells.data();
        R.r.nrows = 1;
        R.r.kept_rows = kept;
        c->yieldDevice++;
        return NGX_OK;
    }

    // ---- projection: scan, emit
    uint64_t m = n;
    if (a.keepBits) {
        uint64_t* base = c->yBase.get<uint64_t>(chunks + 1);
        uint64_t* tiles = c->yTiles.get<uint64_t>((chunks + kTile - 1) / kTile + 1);
        c->timed("yield_scan", chunks * 16, [&] {
            if (launchScanU64(a.chunkCount, chunks, base, tiles, c->stream)) throw Error{NGX_E_DEVICE, "yield scan"};
        });
        a.chunkBase = base;
        m = readScalar(c, base + chunks);
        if (m > n) throw Error{NGX_E_DEVICE, "yield: inconsistent counts"};
        if (int32_t rc = checkErrs()) return rc;
    }
    bool anyString = false;
    for (int32_t y = 0; y < ny; y++) {
        R.colTypes[y] = typeOf[y];
        anyString |= typeOf[y] == NGX_T_STRING;
    }
    uint64_t strBytes = 0;
    if (m) {
        if (anyString) {
            uint64_t* slen = c->ySlen.get<uint64_t>(m + 1);
            uint64_t* spre = c->ySpre.get<uint64_t>(m + 1);
            uint64_t* stiles = c->yTiles.get<uint64_t>(std::max((m + kTile - 1) / kTile + 1, (chunks + kTile - 1) / kTile + 1));
            a.lenOut = slen;
            c->timed("yield_emit", n / 8 + m * 12, [&] {
                if (launchYieldEmit(a, c->stream)) throw Error{NGX_E_DEVICE, "yield string lengths"};
            });
            c->timed("yield_scan", m * 16, [&] {
                if (launchScanU64(slen, m, spre, stiles, c->stream)) throw Error{NGX_E_DEVICE, "yield string scan"};
            });
            strBytes = readScalar(c, spre + m);
            a.lenOut = nullptr;
            a.strPre = spre;
            a.strOut = c->yStr.get<char>(std::max<uint64_t>(strBytes, 1));
        }
        a.cells = c->yCells.get<GroupCell>(m * ny);
        c->timed("yield_emit", n / 8 + m * (rowBytes + ny * sizeof(GroupCell)) + strBytes, [&] {
            if (launchYieldEmit(a, c->stream)) throw Error{NGX_E_DEVICE, "yield emit"};
        });
    }
    finishCells(c, R, a.cells, m * ny, a.strOut, strBytes, [&] {
        HIP_OK(hipMemcpyAsync(errs, errDev, sizeof errs, hipMemcpyDeviceToHost, c->stream));
    });
    if (errs[0] || errs[1]) {                                     // a yield failed on a kept row: no row is returned
        R.cells.clear();
        R.strings.clear();
        R.r.cells = nullptr, R.r.strings = nullptr, R.r.strings_len = 0;
        return fail(c, NGX_E_UNSUPPORTED, errs[1] ? "yield: an expression needs a host-only construct" : kRowFailed);
    }
    R.r.nrows = m;
    R.r.kept_rows = m;
    c->yieldDevice++;
    return NGX_OK;
}

}  // namespace

extern "C" int32_t ngx_go_yield(ngx_ctx* c, const ngx_go_result* r, const ngx_yield_plan* plan, ngx_yield_result** out) {
    if (!c || !r || !plan || !out) return NGX_E_BAD_ARGUMENT;
    // after a failure no kernel is left reading the descriptors
    return abiCall<YieldResultHolder>(c, out, OnFail::kSync, [&](YieldResultHolder& R) { return yieldOp(c, r, plan, R); });
}

extern "C" void ngx_yield_result_free(ngx_yield_result* r) {
    if (r) delete reinterpret_cast<YieldResultHolder*>(r);
}
