// Host AddressSanitizer / UndefinedBehaviorSanitizer run of the library's host-side C++ (the KV ->
// columnar exporter, the snapshot file reader / writer with its consistency checks, the expression
// decoder / pushdown rewrite / bytecode compiler, the synthetic generator) and of the oracle, built by
// tools/san/Makefile with -fsanitize=address,undefined and run by tests/test_sanitizers.py. The device
// side is not here: GPU sanitizers are not available on the pool.
//
// usage: san_driver <dir> [scale]
//   <dir>/go_*.bin     orc_go request blobs over the RMAT space (oracle.go_request)
//   <dir>/expr_*.bin   encoded expressions: seeds of the decoder / compiler fuzz loop
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../nebula_amd/csrc/exprc.h"
#include "../../nebula_amd/csrc/ngx_internal.h"

namespace ngx {
struct DeviceGraph {};                      // engine_ctx.h's is not linked: Space only holds the pointer
}

extern "C" {
typedef struct {
    uint64_t n;
    uint8_t* keys;
    uint64_t* key_off;
    uint8_t* vals;
    uint64_t* val_off;
} ngd_rows;
int32_t ngd_rmat(int32_t scale, int32_t ef, double A, double B, double C, uint64_t seed, int32_t num_parts,
                 int32_t etype, int32_t with_in, int32_t with_tag, int32_t tag, int32_t rank, int32_t world,
                 int32_t threads, ngd_rows* out);
void ngd_free(ngd_rows* r);
typedef struct {
    uint64_t nv;
    int32_t* vpart;
    int64_t* vid;
    int32_t nslots;
    int32_t etype[2];
    uint64_t ne[2];
    uint64_t* off[2];
    int64_t* dst[2];
    int64_t* p0[2];
    int64_t* p1[2];
} ngd_csr;
int32_t ngd_rmat_csr(int32_t scale, int32_t ef, double A, double B, double C, uint64_t seed, int32_t num_parts,
                     int32_t etype, int32_t with_in, int32_t rank, int32_t world, int32_t threads, ngd_csr* out);
void ngd_csr_free(ngd_csr* c);
void* orc_engine_new();
void orc_engine_free(void* e);
void orc_buf_free(void* p);
void orc_set_flags(void* e, int32_t maxHandlers, int32_t minVertices, int32_t maxEdges, int64_t nowSec, int32_t threads);
void orc_add_space(void* e, int32_t space, int32_t numParts);
int32_t orc_add_schema(void* e, int32_t space, int32_t isEdge, int32_t id, const char* name, int64_t ver,
                       int32_t nfields, const char** names, const int32_t* types, const char* ttlCol, int64_t ttlDur);
void orc_put_kv(void* e, int32_t space, uint64_t n, const uint8_t* keys, const uint64_t* koff, const uint8_t* vals,
                const uint64_t* voff);
void orc_finalize(void* e, int32_t threads);
char* orc_go(void* e, int32_t space, const uint8_t* blob, uint64_t len, uint64_t* outLen);
char* orc_expr_eval(const uint8_t* buf, uint64_t len, uint64_t* outLen);
char* orc_expr_roundtrip(const uint8_t* buf, uint64_t len, uint64_t* outLen);
}

using namespace ngx;

namespace {

int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
    std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); failures++; } } while (0)

constexpr int32_t kSpace = 1, kParts = 10, kEdge = 1, kTag = 10;   // datagen.py RMAT_*

std::string readFile(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    std::ostringstream s;
    s << f.rdbuf();
    return s.str();
}

std::vector<std::string> listDir(const std::string& dir, const std::string& prefix) {
    std::vector<std::string> out;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            std::string n = e->d_name;
            if (n.rfind(prefix, 0) == 0) out.push_back(dir + "/" + n);
        }
        closedir(d);
    }
    std::sort(out.begin(), out.end());
    return out;
}

void addSchemas(Space& sp) {
    auto add = [&](bool edge, int32_t id, const char* name, std::vector<FieldDef> f) {
        SchemaDef s;
        s.fields = std::move(f);
        auto& set = edge ? sp.edges[id] : sp.tags[id];
        set.id = id;
        set.name = name;
        set.versions[0] = s;
        if (edge) { sp.edgeByName[name] = id; sp.edgeOrder.push_back(name); }
        else sp.tagByName[name] = id;
    };
    add(true, kEdge, "e", {{"p0", T_INT}, {"p1", T_INT}});
    add(false, kTag, "vt", {{"v0", T_INT}, {"name", T_STRING}});
}

// the rows of parts this rank owns (part % world == rank), as ngx_load_kv stages them
void stage(Space& sp, const ngd_rows& r, int32_t rank, int32_t world) {
    auto& st = sp.staged;
    st = StagedRows{};
    st.voff.push_back(0);
    for (uint64_t i = 0; i < r.n; i++) {
        const uint8_t* k = r.keys + r.key_off[i];
        const uint64_t kl = r.key_off[i + 1] - r.key_off[i];
        int32_t item;
        std::memcpy(&item, k, 4);
        if ((item >> 8) % world != rank) continue;
        st.koff.push_back(st.keys.size());
        st.klen.push_back(static_cast<uint32_t>(kl));
        st.keys.insert(st.keys.end(), k, k + kl);
        st.vals.insert(st.vals.end(), r.vals + r.val_off[i], r.vals + r.val_off[i + 1]);
        st.voff.push_back(st.vals.size());
    }
}

// export every shard of a `world`-rank commit, resolve destination rows with all vertex tables
std::vector<HostGraph> exportWorld(const ngd_rows& r, int32_t world) {
    std::vector<HostGraph> gs(world);
    std::vector<std::vector<std::pair<int32_t, int64_t>>> tables(world);
    for (int32_t w = 0; w < world; w++) {
        Space sp;
        sp.id = kSpace;
        sp.numParts = kParts;
        addSchemas(sp);
        stage(sp, r, w, world);
        Error e = exportSnapshot(sp, w, world, gs[w]);
        CHECK(e.code == NGX_OK, "export rank %d/%d: %s", w, world, e.msg.c_str());
        for (size_t i = 0; i < gs[w].vid.size(); i++) tables[w].push_back({gs[w].vpart[i], gs[w].vid[i]});
    }
    for (int32_t w = 0; w < world; w++) {
        Space sp;
        sp.id = kSpace;
        sp.numParts = kParts;
        addSchemas(sp);
        resolveDstRows(sp, gs[w], tables, world);
        gs[w].gbase = gs[w].shardBase[w];                    // as ngx_commit places the shard
        gs[w].commitDigest = tablesDigest(tables, std::vector<uint64_t>(tables.size(), 7));
    }
    return gs;
}

void snapshots(const ngd_rows& r, const std::string& dir) {
    for (int32_t world : {1, 3}) {
        std::vector<HostGraph> gs = exportWorld(r, world);
        uint64_t edges = 0;
        for (auto& g : gs) edges += g.edges;
        CHECK(edges > 0, "world %d exported no edges", world);
        for (int32_t w = 0; w < world; w++) {
            Space sp;
            sp.id = kSpace;
            sp.numParts = kParts;
            addSchemas(sp);
            const std::string path = dir + "/snap_" + std::to_string(world) + "_" + std::to_string(w) + ".ngx";
            Error e = writeSnapshotFile(sp, gs[w], w, world, path, "san");
            CHECK(e.code == NGX_OK, "write %s: %s", path.c_str(), e.msg.c_str());
            HostGraph back;
            std::string tag;
            e = readSnapshotFile(sp, path, w, world, back, tag);
            CHECK(e.code == NGX_OK && tag == "san", "read %s: %s", path.c_str(), e.msg.c_str());
            CHECK(back.vid == gs[w].vid && back.vpart == gs[w].vpart && back.edges == gs[w].edges &&
                  back.commitDigest == gs[w].commitDigest, "round trip of %s", path.c_str());
            // damaged files: truncations and byte flips are refused with an error or (a flipped value
            // byte) read back; neither may touch memory out of bounds
            const std::string bytes = readFile(path);
            std::mt19937_64 rng(world * 131 + w);
            const std::string bad = path + ".bad";
            for (int k = 0; k < 48; k++) {
                std::string b = bytes;
                if (k < 8) b.resize(b.size() * k / 8);
                else for (int f = 0; f < 1 + k % 4; f++) b[rng() % b.size()] ^= static_cast<char>(1 + rng() % 255);
                { std::ofstream o(bad, std::ios::binary); o.write(b.data(), static_cast<std::streamsize>(b.size())); }
                HostGraph g2;
                e = readSnapshotFile(sp, bad, w, world, g2, tag);
                if (k < 8) CHECK(e.code != NGX_OK, "truncated snapshot (%d/8) accepted", k);
            }
            std::remove(bad.c_str());
            std::remove(path.c_str());
        }
    }
}

// The KV export (exportSnapshot over ngd_rmat's reference-format rows, at a size that takes its parallel
// classify and bucketed sort: > 64 K rows) against the generator's own CSR of the same graph (ngd_rmat_csr,
// pinned against the KV rows by tests/test_datagen_csr.py): vertex table, per slot the offsets, dst and
// both prop columns, equal.
void exportMatchesCsr(int scale) {
    ngd_rows r{};
    CHECK(ngd_rmat(scale, 8, 0.57, 0.19, 0.19, 77, kParts, kEdge, 1, 0, kTag, 0, 1, 4, &r) == 0, "rmat rows");
    Space sp;
    sp.id = kSpace;
    sp.numParts = kParts;
    addSchemas(sp);
    stage(sp, r, 0, 1);
    HostGraph g;
    Error e = exportSnapshot(sp, 0, 1, g);
    CHECK(e.code == NGX_OK, "export: %s", e.msg.c_str());
    ngd_csr c{};
    CHECK(ngd_rmat_csr(scale, 8, 0.57, 0.19, 0.19, 77, kParts, kEdge, 1, 0, 1, 4, &c) == 0, "rmat csr");
    CHECK(g.vid.size() == c.nv, "vertex count %lu vs %lu", static_cast<unsigned long>(g.vid.size()), static_cast<unsigned long>(c.nv));
    bool same = g.vid.size() == c.nv;
    for (uint64_t i = 0; same && i < c.nv; i++) same = g.vid[i] == c.vid[i] && g.vpart[i] == c.vpart[i];
    CHECK(same, "vertex tables differ");
    CHECK(static_cast<int32_t>(g.slots.size()) == c.nslots, "slot count");
    for (int32_t k = 0; k < c.nslots && k < static_cast<int32_t>(g.slots.size()); k++) {
        // the export orders slots by signed type (negative first); match by type
        int32_t j = -1;
        for (int32_t q = 0; q < c.nslots; q++) if (c.etype[q] == g.slots[k].etype) j = q;
        CHECK(j >= 0, "slot %d type %d missing", k, g.slots[k].etype);
        if (j < 0) continue;
        const HostSlot& hs = g.slots[k];
        bool ok = hs.dst.size() == c.ne[j] && hs.off.size() == c.nv + 1 && hs.cols.size() == 2;
        for (uint64_t v = 0; ok && v <= c.nv; v++) ok = hs.off[v] == c.off[j][v];
        for (uint64_t i = 0; ok && i < c.ne[j]; i++)
            ok = hs.dst[i] == c.dst[j][i] && hs.cols[0].i64[i] == c.p0[j][i] && hs.cols[1].i64[i] == c.p1[j][i];
        CHECK(ok, "slot %d (type %d): export and generator CSR differ", k, hs.etype);
    }
    std::printf("export == generator csr: %lu rows, %lu vertices, %lu edges\n", static_cast<unsigned long>(r.n),
                static_cast<unsigned long>(c.nv), static_cast<unsigned long>(g.edges));
    ngd_csr_free(&c);
    ngd_free(&r);
}

void compileBoth(const ExprNode& n, const Space& sp) {
    std::string err;
    StorageCtx sc;
    sc.sp = &sp;
    sc.haveEdgeContexts = true;
    sc.edgeMap["e"] = kEdge;
    Program p;
    (void)compileStorage(n, sc, p, err);
    GraphdCtx gc;
    gc.sp = &sp;
    gc.aliasType["e"] = kEdge;
    gc.direction = 0;
    gc.nEdgeTypes = 1;
    gc.respSchema[kEdge]["p0"] = T_INT;
    gc.respSchema[kEdge]["p1"] = T_INT;
    Program q;
    (void)compileGraphd(n, gc, q, err);
    for (const Insn& in : q.code) (void)in;
    // the pipe form: $-.x / $var.x read from an input table (OP_INPUT)
    static const std::map<std::string, int32_t> inputCols = {{"a", 0}, {"b", 1}, {"id", 2}};
    gc.inputCols = &inputCols;
    Program q2;
    (void)compileGraphd(n, gc, q2, err);
    (void)exprType(n, sp);
}

void expressions(const std::string& dir) {
    Space sp;
    sp.id = kSpace;
    sp.numParts = kParts;
    addSchemas(sp);
    std::mt19937_64 rng(7);
    size_t decoded = 0, tried = 0;
    for (const std::string& f : listDir(dir, "expr_")) {
        const std::string seed = readFile(f);
        std::string err;
        auto n = decodeExpr(reinterpret_cast<const uint8_t*>(seed.data()), seed.size(), err);
        CHECK(n != nullptr, "seed %s does not decode: %s", f.c_str(), err.c_str());
        if (!n) continue;
        CHECK(encodeExpr(*n) == seed, "seed %s: encode(decode(x)) != x", f.c_str());
        compileBoth(*n, sp);
        uint64_t len = 0;
        orc_buf_free(orc_expr_eval(reinterpret_cast<const uint8_t*>(seed.data()), seed.size(), &len));
        for (int k = 0; k < 300; k++) {
            std::string b = seed;
            const int kind = static_cast<int>(rng() % 4);
            if (kind == 0 && !b.empty()) b.resize(rng() % b.size());
            else if (kind == 1 && !b.empty()) b[rng() % b.size()] = static_cast<char>(rng());
            else if (kind == 2) b.insert(b.begin() + static_cast<long>(rng() % (b.size() + 1)), static_cast<char>(rng()));
            else if (!b.empty()) b[rng() % b.size()] ^= static_cast<char>(1u << (rng() % 8));
            tried++;
            auto m = decodeExpr(reinterpret_cast<const uint8_t*>(b.data()), b.size(), err);
            // the oracle decodes every mutation; it evaluates only the seeds (a mutated literal can ask
            // the reference's lpad for 2^60 bytes, which it would try to build)
            uint64_t len = 0;
            orc_buf_free(orc_expr_roundtrip(reinterpret_cast<const uint8_t*>(b.data()), b.size(), &len));
            if (!m) continue;
            decoded++;
            const std::string again = encodeExpr(*m);
            auto c = cloneExpr(*m);
            CHECK(encodeExpr(*c) == again, "clone of a mutated expression differs");
            (void)rewritePushdown(*c);
            compileBoth(*m, sp);
            compileBoth(*c, sp);
        }
    }
    std::printf("expressions: %zu mutations, %zu decoded\n", tried, decoded);
}

void oracleRuns(const ngd_rows& r, const std::string& dir) {
    void* e = orc_engine_new();
    orc_set_flags(e, 10, 3, 2147483647, 0, 4);
    orc_add_space(e, kSpace, kParts);
    const char* en[] = {"p0", "p1"};
    const int32_t et[] = {T_INT, T_INT};
    orc_add_schema(e, kSpace, 1, kEdge, "e", 0, 2, en, et, "", 0);
    const char* tn[] = {"v0", "name"};
    const int32_t tt[] = {T_INT, T_STRING};
    orc_add_schema(e, kSpace, 0, kTag, "vt", 0, 2, tn, tt, "", 0);
    orc_put_kv(e, kSpace, r.n, r.keys, r.key_off, r.vals, r.val_off);
    orc_finalize(e, 4);
    int n = 0;
    for (const std::string& f : listDir(dir, "go_")) {
        const std::string b = readFile(f);
        uint64_t len = 0;
        char* out = orc_go(e, kSpace, reinterpret_cast<const uint8_t*>(b.data()), b.size(), &len);
        CHECK(out != nullptr && len > 0, "orc_go %s returned nothing", f.c_str());
        orc_buf_free(out);
        n++;
    }
    std::printf("oracle: %d GO requests\n", n);
    orc_engine_free(e);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: san_driver <dir> [scale]\n"); return 2; }
    const std::string dir = argv[1];
    const int scale = argc > 2 ? std::atoi(argv[2]) : 10;
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    ngd_rows r{};
    if (ngd_rmat(scale, 8, 0.57, 0.19, 0.19, 42, kParts, kEdge, 1, 1, kTag, 0, 1, 4, &r) != 0) return 2;
    std::printf("rmat scale %d: %lu rows\n", scale, static_cast<unsigned long>(r.n));
    snapshots(r, dir);
    std::printf("snapshots done\n");
    exportMatchesCsr(13);
    expressions(dir);
    oracleRuns(r, dir);
    ngd_free(&r);
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
