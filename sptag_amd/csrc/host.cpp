/* sptag_amd host library — implements the C-ABI in include/sptag_amd.h.
 *
 * Host code is C++ (as the reference's is); all compute runs in the HIP
 * kernels of kernels.hip. There is NO CPU search path here: if the HIP
 * runtime or device is unavailable, every search call fails loudly with
 * SPTAG_AMD_ERR_NOGPU.
 *
 * File formats are byte-compatible with the reference
 * (/root/reference/AnnService):
 *   vectors.bin  [int32 R][int32 C][row-major T]      Dataset.h:146
 *   tree.bin     [int32 #trees][int32 roots x #]
 *                [int32 count][{centerid,childStart,childEnd} x count]
 *                                                     BKTree.h:640-686
 *   graph.bin    [int32 R][int32 deg][int32 adj RxD]  NeighborhoodGraph.h:607
 *   deletes.bin  [int32 count][int32 R][int32 1][int8 x R]  Labelset.h:78
 *   indexloader.ini                                   VectorIndex.cpp:198-222
 */
#include "../../include/sptag_amd.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cctype>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "plan.h"

using namespace sptag_amd;

namespace {

/* Every device allocation of the host code lives in one of these, so any
 * early return releases it. Move-only; frees in the destructor. An empty
 * buffer makes no HIP call, so a handle created on a machine without a GPU
 * is freed without touching the runtime. */
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    /* drop the old block, then allocate exactly `bytes` */
    hipError_t alloc(size_t bytes)
    {
        reset();
        hipError_t e = hipMalloc(&p_, bytes);
        if (e == hipSuccess) cap_ = bytes; else p_ = nullptr;
        return e;
    }
    /* grow-only: a block that is already large enough is kept */
    hipError_t ensure(size_t bytes) { return cap_ >= bytes ? hipSuccess : alloc(bytes); }
    template <class T = void> T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};

/* the start/stop event pair that times a kernel pass; created on first use */
struct DevEvents {
    hipEvent_t start = nullptr, stop = nullptr;
    DevEvents() = default;
    DevEvents(const DevEvents&) = delete;
    DevEvents& operator=(const DevEvents&) = delete;
    ~DevEvents()
    {
        if (start) (void)hipEventDestroy(start);
        if (stop) (void)hipEventDestroy(stop);
    }
    void ensure()
    {
        if (!start) { (void)hipEventCreate(&start); (void)hipEventCreate(&stop); }
    }
};

struct HostIndex {
    int device = 0;
    int algo = ALGO_BKT;
    int vt = VT_FLOAT, dm = DM_L2;
    int32_t n = 0, dim = 0, deg = 0, ntrees = 0, n_tree_nodes = 0;
    int32_t default_maxcheck = DEFAULT_MAXCHECK;
    int32_t init_pivots = INIT_PIVOTS, other_pivots = OTHER_PIVOTS;
    int32_t nobetter_threshold = 3;  /* KDT ParameterDefinitionList */
    bool has_deleted = false;
    /* the index on the device */
    DevBuf d_vectors, d_graph, d_tree, d_tree_start, d_deleted;
    /* host copies kept for save_index and shard assembly */
    std::vector<char> h_vectors;
    std::vector<int32_t> h_graph, h_tree, h_tree_start;
    std::vector<uint8_t> h_deleted;
    int64_t deleted_count = 0;
    std::mutex lock;
    /* cached per-handle search scratch (grow-only) */
    DevBuf d_visited, d_oflow, d_stats, d_gng, d_gspt, d_redo, d_gspt0, d_gng0;
    DevEvents ev;
    double last_kernel_ms = 0;
    long long last_checked = 0, last_popped = 0;

    size_t esz() const { return vt == VT_FLOAT ? 4 : 1; }
    IndexParams params() const
    {
        return {algo, dim, esz(), init_pivots, other_pivots, nobetter_threshold};
    }
    DevIndex dev() const {
        DevIndex di;
        di.vectors = d_vectors.as();
        di.graph = d_graph.as<int32_t>();
        di.tree_nodes = d_tree.as<int32_t>();
        di.tree_start = d_tree_start.as<int32_t>();
        di.deleted = d_deleted.as<uint8_t>();
        di.n = n; di.dim = dim; di.deg = deg; di.ntrees = ntrees;
        di.n_tree_nodes = n_tree_nodes;
        di.has_deleted = has_deleted ? 1 : 0;
        di.algo = algo;
        return di;
    }
};

#define HIP_OR_FAIL(expr, ret)                                              \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) {                                             \
            fprintf(stderr, "sptag_amd: HIP error %s at %s:%d\n",           \
                    hipGetErrorString(_e), __FILE__, __LINE__);             \
            return ret;                                                     \
        }                                                                   \
    } while (0)

/* allocate `b` at `bytes` and fill it from host memory */
int dev_upload(DevBuf& b, const void* src, size_t bytes)
{
    HIP_OR_FAIL(b.alloc(bytes), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(hipMemcpy(b.as(), src, bytes, hipMemcpyHostToDevice),
                SPTAG_AMD_ERR_NOGPU);
    return SPTAG_AMD_OK;
}

bool read_file(const std::string& path, std::vector<char>& out)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize((size_t)sz);
    bool ok = fread(out.data(), 1, (size_t)sz, f) == (size_t)sz;
    fclose(f);
    return ok;
}

/* SimpleIniReader-compatible lookup (reference src/Helper/
 * SimpleIniReader.cpp): case-insensitive section and key names, leading/
 * trailing whitespace around the key and value tolerated, ';' comment
 * lines skipped. This is the drop-in seam, so it accepts what the
 * reference's own parser would. */
static bool ieq(const std::string& a, const std::string& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (tolower((unsigned char)a[i]) != tolower((unsigned char)b[i]))
            return false;
    return true;
}

static std::string trim(const std::string& s)
{
    size_t b = s.find_first_not_of(" \t\r");
    if (b == std::string::npos) return "";
    size_t e = s.find_last_not_of(" \t\r");
    return s.substr(b, e - b + 1);
}

bool ini_get(const std::string& text, const char* section, const char* key,
             std::string& out)
{
    bool in_section = false;
    size_t p = 0;
    while (p < text.size()) {
        size_t eol = text.find('\n', p);
        if (eol == std::string::npos) eol = text.size();
        std::string line = trim(text.substr(p, eol - p));
        p = eol + 1;
        if (line.empty() || line[0] == ';') continue;
        if (line.front() == '[') {
            size_t close = line.find(']');
            if (close == std::string::npos) continue;
            in_section = ieq(trim(line.substr(1, close - 1)), section);
            continue;
        }
        if (!in_section) continue;
        size_t eq = line.find('=');
        if (eq == std::string::npos) continue;
        if (ieq(trim(line.substr(0, eq)), key)) {
            out = trim(line.substr(eq + 1));
            return true;
        }
    }
    return false;
}

int upload(HostIndex* ix)
{
    HIP_OR_FAIL(hipSetDevice(ix->device), SPTAG_AMD_ERR_NOGPU);
    int rc = dev_upload(ix->d_vectors, ix->h_vectors.data(), ix->h_vectors.size());
    if (rc == SPTAG_AMD_OK)
        rc = dev_upload(ix->d_graph, ix->h_graph.data(), ix->h_graph.size() * 4);
    if (rc == SPTAG_AMD_OK)
        rc = dev_upload(ix->d_tree, ix->h_tree.data(), ix->h_tree.size() * 4);
    if (rc == SPTAG_AMD_OK)
        rc = dev_upload(ix->d_tree_start, ix->h_tree_start.data(),
                        ix->h_tree_start.size() * 4);
    if (rc == SPTAG_AMD_OK && ix->has_deleted)
        rc = dev_upload(ix->d_deleted, ix->h_deleted.data(), ix->h_deleted.size());
    return rc;
}

/* device vids and dists of a top-k result, n entries each (grow-only) */
struct TopkOut {
    DevBuf v, d;
    int32_t* vids() const { return v.as<int32_t>(); }
    float* dists() const { return d.as<float>(); }
    int ensure(size_t n)
    {
        HIP_OR_FAIL(v.ensure(n * 4), SPTAG_AMD_ERR_OOM);
        HIP_OR_FAIL(d.ensure(n * 4), SPTAG_AMD_ERR_OOM);
        return SPTAG_AMD_OK;
    }
    int download(int32_t* out_vids, float* out_dists, size_t n) const
    {
        HIP_OR_FAIL(hipMemcpy(out_vids, v.as(), n * 4, hipMemcpyDeviceToHost),
                    SPTAG_AMD_ERR_NOGPU);
        HIP_OR_FAIL(hipMemcpy(out_dists, d.as(), n * 4, hipMemcpyDeviceToHost),
                    SPTAG_AMD_ERR_NOGPU);
        return SPTAG_AMD_OK;
    }
};

/* Every environment variable the search path reads. Read once per search
 * and never cached: callers change the environment between searches. */
SearchKnobs read_knobs()
{
    SearchKnobs k;
    if (const char* e = getenv("SPTAG_AMD_NG_CAP"))
        k.ng_cap_override = std::max(1, atoi(e));   /* "0" is an override too */
    if (const char* e = getenv("SPTAG_AMD_NG_GLEVELS")) k.ng_glevels = atoi(e);
    k.prof = getenv("SPTAG_AMD_PROF") != nullptr;
    k.debug = getenv("SPTAG_AMD_DEBUG") != nullptr;
    return k;
}

/* read cursor over a file's bytes: take() refuses to run past the end */
struct Cursor {
    const char* p;
    size_t left;
    explicit Cursor(const std::vector<char>& b) : p(b.data()), left(b.size()) {}
    const char* take(size_t bytes)
    {
        if (bytes > left) return nullptr;
        const char* r = p;
        p += bytes;
        left -= bytes;
        return r;
    }
    bool i32(int32_t& v)
    {
        const char* s = take(4);
        if (s) memcpy(&v, s, 4);
        return s != nullptr;
    }
};

struct Part { const void* p; size_t n; };

/* write the parts back to back; false on any short write */
bool write_file(const std::string& path, std::initializer_list<Part> parts)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    bool ok = true;
    for (const Part& s : parts)
        ok = ok && (s.n == 0 || fwrite(s.p, 1, s.n, f) == s.n);
    return fclose(f) == 0 && ok;
}

}  // namespace

struct SptagAmdIndex : HostIndex {};

/* The one place that validates arguments and builds a handle; `tree_nodes`
 * holds 3 int32 per node for BKT and 4 for KDT. */
static SptagAmdIndex* create_index(int algo, int32_t n, int32_t dim, int valuetype,
                                   int distmethod, const void* vectors,
                                   int32_t ntrees, const int32_t* tree_start,
                                   int32_t n_tree_nodes, const int32_t* tree_nodes,
                                   int32_t degree, const int32_t* graph,
                                   const uint8_t* deleted, int device)
{
    if (n <= 0 || dim <= 0 || dim > MAX_DIM || degree <= 0 || degree > MAX_DEG ||
        ntrees <= 0 || n_tree_nodes <= 0)
        return nullptr;
    if (valuetype == SPTAG_AMD_VT_INT8 && (int64_t)dim * 254 * 254 >= (1ll << 24)) {
        /* beyond this the int8 distances stop being exact integers in float */
        fprintf(stderr, "sptag_amd: int8 dim %d exceeds exact-float range\n", dim);
        return nullptr;
    }
    std::unique_ptr<SptagAmdIndex> ix(new SptagAmdIndex());
    ix->device = device;
    ix->algo = algo;
    ix->vt = valuetype;
    ix->dm = distmethod;
    ix->n = n; ix->dim = dim; ix->deg = degree;
    ix->ntrees = ntrees;
    ix->h_vectors.assign((const char*)vectors,
                         (const char*)vectors + (size_t)n * dim * ix->esz());
    ix->h_graph.assign(graph, graph + (size_t)n * degree);
    ix->h_tree_start.assign(tree_start, tree_start + ntrees);
    const size_t width = algo == ALGO_KDT ? 4 : 3;
    ix->h_tree.assign(tree_nodes, tree_nodes + (size_t)n_tree_nodes * width);
    /* BKTree.h:683: append sentinel if the stored array does not end with
     * centerid == -1 */
    if (algo == ALGO_BKT && ix->h_tree[(size_t)(n_tree_nodes - 1) * 3] != -1) {
        ix->h_tree.insert(ix->h_tree.end(), 3, -1);
        n_tree_nodes += 1;
    }
    ix->n_tree_nodes = n_tree_nodes;
    if (deleted) {
        ix->h_deleted.assign(deleted, deleted + n);
        for (int32_t i = 0; i < n; i++) ix->deleted_count += deleted[i] ? 1 : 0;
        ix->has_deleted = ix->deleted_count > 0;
    }
    /* without a GPU the handle still supports metadata queries + save_index;
     * search fails with ERR_NOGPU. */
    if (sptag_amd_gpu_available() && upload(ix.get()) != SPTAG_AMD_OK) return nullptr;
    return ix.release();
}

extern "C" {

int sptag_amd_gpu_available(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

const char* sptag_amd_build_info(void)
{
    return "sptag_amd gfx950 v1 (BKT search; HIP " __DATE__ ")";
}

SptagAmdIndex* sptag_amd_create_index(int32_t n, int32_t dim, int valuetype,
                                      int distmethod, const void* vectors,
                                      int32_t ntrees, const int32_t* tree_start,
                                      int32_t n_tree_nodes, const int32_t* tree_nodes,
                                      int32_t degree, const int32_t* graph,
                                      const uint8_t* deleted, int device)
{
    return create_index(ALGO_BKT, n, dim, valuetype, distmethod, vectors, ntrees,
                        tree_start, n_tree_nodes, tree_nodes, degree, graph,
                        deleted, device);
}

SptagAmdIndex* sptag_amd_create_index_kdt(int32_t n, int32_t dim, int valuetype,
                                          int distmethod, const void* vectors,
                                          int32_t ntrees, const int32_t* tree_start,
                                          int32_t n_tree_nodes, const void* kdt_nodes,
                                          int32_t degree, const int32_t* graph,
                                          const uint8_t* deleted, int device)
{
    return create_index(ALGO_KDT, n, dim, valuetype, distmethod, vectors, ntrees,
                        tree_start, n_tree_nodes, (const int32_t*)kdt_nodes, degree,
                        graph, deleted, device);
}

SptagAmdIndex* sptag_amd_load_index(const char* folder, int device)
{
    std::string dir(folder);
    if (!dir.empty() && dir.back() != '/') dir += '/';

    std::vector<char> raw;
    if (!read_file(dir + "indexloader.ini", raw)) return nullptr;
    std::string ini(raw.begin(), raw.end());

    std::string val;
    int algo = ALGO_BKT;
    if (ini_get(ini, "Index", "IndexAlgoType", val)) {
        if (val == "BKT") algo = ALGO_BKT;
        else if (val == "KDT") algo = ALGO_KDT;
        else {
            fprintf(stderr, "sptag_amd: IndexAlgoType %s not supported\n",
                    val.c_str());
            return nullptr;
        }
    }
    int vt = VT_FLOAT, dm = DM_L2;
    if (ini_get(ini, "Index", "ValueType", val)) {
        if (val == "Float") vt = VT_FLOAT;
        else if (val == "Int8") vt = VT_INT8;
        else {
            fprintf(stderr, "sptag_amd: ValueType %s not supported\n", val.c_str());
            return nullptr;
        }
    }
    if (ini_get(ini, "Index", "DistCalcMethod", val)) {
        if (val == "L2") dm = DM_L2;
        else if (val == "Cosine" || val == "InnerProduct") dm = DM_COSINE;
        else {
            fprintf(stderr, "sptag_amd: DistCalcMethod %s not supported\n", val.c_str());
            return nullptr;
        }
    }

    std::vector<char> vb, tb, gb, db;
    if (!read_file(dir + "vectors.bin", vb) || !read_file(dir + "tree.bin", tb) ||
        !read_file(dir + "graph.bin", gb))
        return nullptr;
    bool have_del = read_file(dir + "deletes.bin", db);

    /* every header field and body is taken through a cursor, so a short or
     * empty file is a failed load, never a read past the buffer */
    Cursor vc(vb), tc(tb), gc(gb);
    int32_t n = 0, dim = 0, ntrees = 0, nnodes = 0, gn = 0, deg = 0;
    const char *vecs = nullptr, *tstart = nullptr, *tnodes = nullptr, *adj = nullptr;
    const size_t esz = vt == VT_FLOAT ? 4 : 1, node_bytes = algo == ALGO_KDT ? 16 : 12;
    auto refuse = [](const char* file) -> SptagAmdIndex* {
        fprintf(stderr, "sptag_amd: %s is truncated or malformed\n", file);
        return nullptr;
    };
    if (!vc.i32(n) || !vc.i32(dim) || n <= 0 || dim <= 0 || dim > MAX_DIM ||
        !(vecs = vc.take((size_t)n * dim * esz)))
        return refuse("vectors.bin");
    if (!tc.i32(ntrees) || ntrees <= 0 || !(tstart = tc.take((size_t)ntrees * 4)) ||
        !tc.i32(nnodes) || nnodes <= 0 ||
        !(tnodes = tc.take((size_t)nnodes * node_bytes)))
        return refuse("tree.bin");
    if (!gc.i32(gn) || !gc.i32(deg) || deg <= 0 || deg > MAX_DEG)
        return refuse("graph.bin");
    if (gn != n) {
        fprintf(stderr, "sptag_amd: graph rows %d != vectors %d\n", gn, n);
        return nullptr;
    }
    if (!(adj = gc.take((size_t)n * deg * 4))) return refuse("graph.bin");
    const uint8_t* del = nullptr;
    if (have_del && db.size() >= 12 + (size_t)n) {
        int32_t delcount = ((const int32_t*)db.data())[0];
        if (delcount > 0) del = (const uint8_t*)db.data() + 12;
    }

    SptagAmdIndex* ix = create_index(algo, n, dim, vt, dm, vecs, ntrees,
                                     (const int32_t*)tstart, nnodes,
                                     (const int32_t*)tnodes, deg,
                                     (const int32_t*)adj, del, device);
    if (!ix) return nullptr;
    if (ini_get(ini, "Index", "ThresholdOfNumberOfContinuousNoBetterPropagation", val))
        ix->nobetter_threshold = atoi(val.c_str());
    if (ini_get(ini, "Index", "MaxCheck", val)) ix->default_maxcheck = atoi(val.c_str());
    if (ini_get(ini, "Index", "NumberOfInitialDynamicPivots", val))
        ix->init_pivots = atoi(val.c_str());
    if (ini_get(ini, "Index", "NumberOfOtherDynamicPivots", val))
        ix->other_pivots = atoi(val.c_str());
    if (ini_get(ini, "Index", "EnableBfs", val) && atoi(val.c_str()) != 0) {
        fprintf(stderr, "sptag_amd: EnableBfs not supported\n");
        sptag_amd_free_index(ix);
        return nullptr;
    }
    return ix;
}

void sptag_amd_free_index(SptagAmdIndex* ix)
{
    if (ix) delete ix;   /* the owners on the handle release the device side */
}

/* host copies of one pass's per-query stats and overflow flags */
struct PassOut {
    int sstride;
    std::vector<int32_t> stats, oflow;
    PassOut(int stride, int32_t nq)
        : sstride(stride), stats((size_t)stride * nq), oflow(nq) {}
};

/* One kernel pass over cfg.nq queries: zero the visited tables, launch
 * between the two events, sync, read back stats and overflow flags, and add
 * the time and the counters of the queries that did not overflow to the
 * handle's last_* figures. With `d_idx` the pass ran on gathered rows, and
 * its results are scattered to d_vids/d_dists before the one sync. */
static int run_pass(SptagAmdIndex* ix, bool heaps_in_lds, const SearchCfg& cfg,
                    const SearchBufs& bufs, PassOut& out,
                    const int32_t* d_idx = nullptr, int32_t* d_vids = nullptr,
                    float* d_dists = nullptr)
{
    const int32_t nq = cfg.nq;
    HIP_OR_FAIL(hipMemsetAsync(bufs.visited, 0, (size_t)nq * cfg.vcap * 4),
                SPTAG_AMD_ERR_NOGPU);
    (void)hipEventRecord(ix->ev.start);
    int err = launch_bkt_search(ix->vt, ix->dm, heaps_in_lds, ix->dev(), cfg, bufs);
    if (err != 0) {
        fprintf(stderr, "sptag_amd: %slaunch failed %d\n",
                heaps_in_lds ? "" : "global-variant ", err);
        return SPTAG_AMD_ERR_INTERNAL;
    }
    (void)hipEventRecord(ix->ev.stop);
    if (d_idx) {
        launch_copy_rows(false, d_vids, bufs.out_vids, cfg.k * 4, d_idx, nq);
        launch_copy_rows(false, d_dists, bufs.out_dists, cfg.k * 4, d_idx, nq);
    }
    HIP_OR_FAIL(hipDeviceSynchronize(), SPTAG_AMD_ERR_NOGPU);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ix->ev.start, ix->ev.stop);
    ix->last_kernel_ms += ms;
    HIP_OR_FAIL(hipMemcpy(out.oflow.data(), bufs.oflow, (size_t)nq * 4,
                          hipMemcpyDeviceToHost), SPTAG_AMD_ERR_NOGPU);
    HIP_OR_FAIL(hipMemcpy(out.stats.data(), bufs.stats, (size_t)nq * out.sstride * 4,
                          hipMemcpyDeviceToHost), SPTAG_AMD_ERR_NOGPU);
    for (int32_t i = 0; i < nq; i++) {
        if (out.oflow[i]) continue;
        ix->last_checked += out.stats[(size_t)out.sstride * i];
        ix->last_popped += out.stats[(size_t)out.sstride * i + 1];
    }
    return SPTAG_AMD_OK;
}

/* SPTAG_AMD_PROF: per-phase cycle sums of one LDS pass (BKT kernels only) */
static void prof_dump(const PassOut& out, int32_t nq, double ms)
{
    enum { NPHASE = 9 };
    static const char* pname[NPHASE] = {
        "seed", "pop", "row", "serial", "cas", "dist", "insert", "tree", "sort"};
    double tot[NPHASE] = {};
    for (int32_t i = 0; i < nq; i++)
        for (int p = 0; p < NPHASE; p++)
            tot[p] += (double)out.stats[(size_t)out.sstride * i + 2 + p];
    double all = 0;
    for (int p = 0; p < NPHASE; p++) all += tot[p];
    fprintf(stderr, "sptag_amd PROF (sum of per-query wave cycles, "
                    "%d queries, kernel %.2f ms):\n", nq, ms);
    for (int p = 0; p < NPHASE; p++)
        fprintf(stderr, "  %-7s %14.0f  (%5.1f%%)\n", pname[p], tot[p],
                all > 0 ? 100.0 * tot[p] / all : 0.0);
    double ngi = 0;
    for (int32_t i = 0; i < nq; i++)
        ngi += (double)out.stats[(size_t)out.sstride * i + 2 + NPHASE];
    fprintf(stderr, "  (insert = ng-heap %14.0f + results-set rest)\n", ngi);
    /* inside seed + tree: the tree heap's inserts and pops, and the leaf
     * branch of SearchTrees (visited CAS + NG insert) */
    static const char* aname[3] = {"spt-insert", "spt-pop", "leaf"};
    for (int a = 0; a < 3; a++) {
        double t = 0;
        for (int32_t i = 0; i < nq; i++)
            t += (double)out.stats[(size_t)out.sstride * i + 3 + NPHASE + a];
        fprintf(stderr, "  (seed+tree: %-10s %14.0f  (%5.1f%%))\n", aname[a], t,
                all > 0 ? 100.0 * t / all : 0.0);
    }
}

/* core search on DEVICE buffers; scratch cached on the handle. */
static int search_device_core(SptagAmdIndex* ix, const void* d_q, int32_t nq,
                              int32_t k, int32_t max_check,
                              int32_t* d_vids, float* d_dists, bool refine = false)
{
    if (max_check <= 0) max_check = ix->default_maxcheck;

    /* 1. plan: every capacity of both passes */
    const SearchKnobs knobs = read_knobs();
    int lds_limit = LDS_PASS_MAX_BYTES;
    (void)hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock,
                                ix->device);
    const SearchPlan plan =
        plan_search(ix->params(), k, max_check, refine, lds_limit, knobs);
    SearchCfg cfg = plan.lds;
    cfg.nq = nq;

    /* 2. scratch of the LDS pass; visited, flags and stats serve both passes */
    HIP_OR_FAIL(ix->d_visited.ensure(nq * plan.visited_bytes), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(ix->d_oflow.ensure((size_t)nq * 4), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(ix->d_stats.ensure((size_t)nq * plan.sstride * 4), SPTAG_AMD_ERR_OOM);
    ix->ev.ensure();
    HIP_OR_FAIL(ix->d_gspt0.ensure(nq * plan.gspt0_bytes), SPTAG_AMD_ERR_OOM);
    if (plan.ng_tail)
        HIP_OR_FAIL(ix->d_gng0.ensure(nq * plan.gng0_bytes), SPTAG_AMD_ERR_OOM);

    SearchBufs bufs;
    bufs.queries = d_q;
    bufs.out_vids = d_vids;
    bufs.out_dists = d_dists;
    bufs.visited = ix->d_visited.as<int32_t>();
    bufs.oflow = ix->d_oflow.as<int32_t>();
    bufs.stats = ix->d_stats.as<int32_t>();
    bufs.gheap_ng = plan.ng_tail ? ix->d_gng0.as() : nullptr;
    bufs.gheap_spt = ix->d_gspt0.as();

    /* 3. LDS pass, 4. pick the reruns */
    ix->last_kernel_ms = 0;
    ix->last_checked = 0;
    ix->last_popped = 0;
    PassOut out(plan.sstride, nq);
    std::vector<int32_t> redo;
    bool all_global = !plan.lds_ok;
    if (plan.lds_ok) {
        int rc = run_pass(ix, true, cfg, bufs, out);
        if (rc != SPTAG_AMD_OK) return rc;
        for (int32_t i = 0; i < nq; i++)
            if (out.oflow[i]) redo.push_back(i);
        if (cfg.prof) prof_dump(out, nq, ix->last_kernel_ms);
        if (!redo.empty() && knobs.debug)
            fprintf(stderr, "sptag_amd: %zu/%d queries overflowed (rerun)\n",
                    redo.size(), nq);
        if (redo.size() * 2 > (size_t)nq) {
            all_global = true;   /* cheaper to redo the whole batch */
            redo.clear();
            ix->last_checked = 0;
            ix->last_popped = 0;
        }
    }

    /* 5. global-heap pass at the reference's capacities */
    int32_t gq_n = all_global ? nq : (int32_t)redo.size();
    if (gq_n == 0) return SPTAG_AMD_OK;
    if (knobs.debug)
        fprintf(stderr, "sptag_amd: global-heap pass for %d/%d queries\n", gq_n, nq);
    SearchCfg c2 = cfg;
    c2.nq = gq_n;
    c2.ng_cap = plan.g_ng_cap;
    c2.spt_cap = plan.g_spt_cap;
    HIP_OR_FAIL(ix->d_gng.ensure(gq_n * plan.gng_bytes), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(ix->d_gspt.ensure(gq_n * plan.gspt_bytes), SPTAG_AMD_ERR_OOM);
    SearchBufs b2 = bufs;
    b2.gheap_ng = ix->d_gng.as();
    b2.gheap_spt = ix->d_gspt.as();
    int32_t* d_idx = nullptr;
    if (!all_global) {
        /* compact the flagged queries on-device */
        size_t row = (size_t)ix->dim * ix->esz();
        size_t qseg = ((size_t)gq_n * row + 15) & ~15ul;  /* align */
        size_t need = (size_t)gq_n * 4 + 16 + qseg + (size_t)gq_n * k * 8;
        HIP_OR_FAIL(ix->d_redo.ensure(need), SPTAG_AMD_ERR_OOM);
        d_idx = ix->d_redo.as<int32_t>();
        char* d_q2 = ix->d_redo.as<char>() + (((size_t)gq_n * 4 + 15) & ~15ul);
        int32_t* d_v2 = (int32_t*)(d_q2 + qseg);
        HIP_OR_FAIL(hipMemcpy(d_idx, redo.data(), (size_t)gq_n * 4,
                              hipMemcpyHostToDevice), SPTAG_AMD_ERR_NOGPU);
        launch_copy_rows(true, d_q2, d_q, (int)row, d_idx, gq_n);
        b2.queries = d_q2;
        b2.out_vids = d_v2;
        b2.out_dists = (float*)(d_v2 + (size_t)gq_n * k);
    }
    int rc = run_pass(ix, false, c2, b2, out, d_idx, d_vids, d_dists);
    if (rc != SPTAG_AMD_OK) return rc;
    /* a query can still overflow at reference capacities only through
     * visited-table saturation (probe give-up) — that would be a silent
     * result truncation, so it is an error, not a degradation. */
    for (int32_t i = 0; i < gq_n; i++) {
        if (out.oflow[i]) {
            fprintf(stderr,
                    "sptag_amd: query overflowed at reference capacities "
                    "(visited-table saturation)\n");
            return SPTAG_AMD_ERR_INTERNAL;
        }
    }
    return SPTAG_AMD_OK;
}

static int check_search_args(SptagAmdIndex* ix, const void* q, int32_t nq, int32_t k)
{
    if (!ix || !q || nq <= 0 || k <= 0 || k > MAX_K) return SPTAG_AMD_ERR_PARAM;
    if (!sptag_amd_gpu_available() || !ix->d_vectors) {
        fprintf(stderr,
                "sptag_amd: search requires a HIP device (%s); no CPU fallback\n",
                sptag_amd_build_info());
        return SPTAG_AMD_ERR_NOGPU;
    }
    return SPTAG_AMD_OK;
}

int sptag_amd_search_batch_device(SptagAmdIndex* ix, const void* d_queries,
                                  int32_t nq, int32_t k, int32_t max_check,
                                  int32_t* d_out_vids, float* d_out_dists)
{
    int rc = check_search_args(ix, d_queries, nq, k);
    if (rc != SPTAG_AMD_OK) return rc;
    std::lock_guard<std::mutex> g(ix->lock);
    HIP_OR_FAIL(hipSetDevice(ix->device), SPTAG_AMD_ERR_NOGPU);
    return search_device_core(ix, d_queries, nq, k, max_check, d_out_vids,
                              d_out_dists);
}

int sptag_amd_search_batch(SptagAmdIndex* ix, const void* queries, int32_t nq,
                           int32_t k, int32_t max_check,
                           int32_t* out_vids, float* out_dists)
{
    int rc = check_search_args(ix, queries, nq, k);
    if (rc != SPTAG_AMD_OK) return rc;
    std::lock_guard<std::mutex> g(ix->lock);
    HIP_OR_FAIL(hipSetDevice(ix->device), SPTAG_AMD_ERR_NOGPU);

    const size_t n = (size_t)nq * k;
    DevBuf d_q;
    TopkOut out;
    if ((rc = dev_upload(d_q, queries, (size_t)nq * ix->dim * ix->esz())) != SPTAG_AMD_OK)
        return rc;
    if ((rc = out.ensure(n)) != SPTAG_AMD_OK) return rc;
    rc = search_device_core(ix, d_q.as(), nq, k, max_check, out.vids(), out.dists());
    return rc != SPTAG_AMD_OK ? rc : out.download(out_vids, out_dists, n);
}

void sptag_amd_last_stats(SptagAmdIndex* ix, double* kernel_ms,
                          long long* checked, long long* popped)
{
    if (!ix) return;
    if (kernel_ms) *kernel_ms = ix->last_kernel_ms;
    if (checked) *checked = ix->last_checked;
    if (popped) *popped = ix->last_popped;
}

struct SptagAmdIterBatch {
    SptagAmdIndex* ix = nullptr;
    int32_t nq = 0, max_check = 0;
    IterPlan plan = {};
    /* queries and persistent traversal state */
    DevBuf d_q, d_ng, d_spt, d_dpq, d_visited, d_state;
    /* per-call outputs; `out` grows with the largest batch asked for */
    TopkOut out;
    DevBuf d_oc, d_or;
};

SptagAmdIterBatch* sptag_amd_iter_create(SptagAmdIndex* ix, const void* queries,
                                         int32_t nq, int32_t max_check)
{
    if (!ix || !queries || nq <= 0) return nullptr;
    if (ix->algo != ALGO_BKT) {
        /* reference parity: KDT::Index<T>::GetIterator logs "ITERATIVE NOT
         * SUPPORT FOR KDT" and returns null (KDTIndex.cpp:322-346) */
        fprintf(stderr, "sptag_amd: iterative search is BKT-only "
                        "(as in the reference: KDTIndex.cpp:322)\n");
        return nullptr;
    }
    if (!sptag_amd_gpu_available() || !ix->d_vectors) {
        fprintf(stderr, "sptag_amd: iterator requires a HIP device\n");
        return nullptr;
    }
    if (max_check <= 0) max_check = ix->default_maxcheck;
    std::unique_ptr<SptagAmdIterBatch> it(new SptagAmdIterBatch());
    it->ix = ix;
    it->nq = nq;
    it->max_check = max_check;
    const IterPlan& p = it->plan = plan_iter(max_check);
    std::vector<IterState> init(nq);
    for (auto& st : init) { st = IterState{}; st.first = 1; }
    const size_t vbytes = (size_t)nq * p.vcap * 4;
    if (dev_upload(it->d_q, queries, (size_t)nq * ix->dim * ix->esz()) != SPTAG_AMD_OK)
        return nullptr;
    HIP_OR_FAIL(it->d_ng.alloc(nq * heap_slab_bytes(p.ng_cap)), nullptr);
    HIP_OR_FAIL(it->d_spt.alloc(nq * heap_slab_bytes(p.spt_cap)), nullptr);
    HIP_OR_FAIL(it->d_dpq.alloc((size_t)nq * (p.dpq_alloc + 1) * 4), nullptr);
    HIP_OR_FAIL(it->d_visited.alloc(vbytes), nullptr);
    HIP_OR_FAIL(hipMemset(it->d_visited.as(), 0, vbytes), nullptr);
    HIP_OR_FAIL(it->d_oc.alloc((size_t)nq * 4), nullptr);
    HIP_OR_FAIL(it->d_or.alloc((size_t)nq * 4), nullptr);
    if (dev_upload(it->d_state, init.data(), (size_t)nq * sizeof(IterState)) !=
        SPTAG_AMD_OK)
        return nullptr;
    return it.release();
}

void sptag_amd_iter_free(SptagAmdIterBatch* it)
{
    if (it) delete it;
}

int sptag_amd_iter_next(SptagAmdIterBatch* it, int32_t batch,
                        int32_t* out_vids, float* out_dists,
                        int32_t* out_counts, int32_t* out_relaxed)
{
    if (!it || batch <= 0 || batch > MAX_K) return SPTAG_AMD_ERR_PARAM;
    SptagAmdIndex* ix = it->ix;
    std::lock_guard<std::mutex> g(ix->lock);
    HIP_OR_FAIL(hipSetDevice(ix->device), SPTAG_AMD_ERR_NOGPU);
    const size_t n = (size_t)it->nq * batch;
    int rc = it->out.ensure(n);
    if (rc != SPTAG_AMD_OK) return rc;
    /* dpq_cap comes out as the ResetResult cap, max(max_check/16, batch) */
    SearchCfg cfg = base_cfg(ix->params(), batch, it->max_check, false);
    cfg.nq = it->nq;
    cfg.vcap = it->plan.vcap;
    cfg.ng_cap = it->plan.ng_cap;
    cfg.spt_cap = it->plan.spt_cap;

    IterBufs ib;
    ib.queries = it->d_q.as();
    ib.gheap_ng = it->d_ng.as();
    ib.gheap_spt = it->d_spt.as();
    ib.dpq = it->d_dpq.as<float>();
    ib.visited = it->d_visited.as<int32_t>();
    ib.state = it->d_state.as<IterState>();
    ib.out_vids = it->out.vids();
    ib.out_dists = it->out.dists();
    ib.out_counts = it->d_oc.as<int32_t>();
    ib.out_relaxed = it->d_or.as<int32_t>();
    int err = launch_bkt_iter(ix->vt, ix->dm, ix->dev(), cfg, ib, batch);
    if (err != 0) {
        fprintf(stderr, "sptag_amd: iter launch failed %d\n", err);
        return SPTAG_AMD_ERR_INTERNAL;
    }
    HIP_OR_FAIL(hipDeviceSynchronize(), SPTAG_AMD_ERR_NOGPU);
    /* The heaps sit at the reference's capacities, so a set overflow flag
     * means the fixed visited table gave up probing (the reference's grows
     * on demand and its iterator runs on past MaxCheck). The kernel has
     * stopped that query early; its short count would read as exhaustion —
     * a silent result truncation, so it is an error, as in the one-shot
     * search. The flag is sticky: every later call fails the same way. */
    std::vector<IterState> st(it->nq);
    HIP_OR_FAIL(hipMemcpy(st.data(), ib.state, (size_t)it->nq * sizeof(IterState),
                          hipMemcpyDeviceToHost), SPTAG_AMD_ERR_NOGPU);
    for (int32_t i = 0; i < it->nq; i++) {
        if (st[i].oflow) {
            fprintf(stderr,
                    "sptag_amd: iterator query %d overflowed at reference "
                    "capacities (visited-table saturation, %d slots); "
                    "create the iterator with a larger MaxCheck\n", i, it->plan.vcap);
            return SPTAG_AMD_ERR_INTERNAL;
        }
    }
    if ((rc = it->out.download(out_vids, out_dists, n)) != SPTAG_AMD_OK) return rc;
    HIP_OR_FAIL(hipMemcpy(out_counts, ib.out_counts, (size_t)it->nq * 4,
                          hipMemcpyDeviceToHost), SPTAG_AMD_ERR_NOGPU);
    if (out_relaxed)
        HIP_OR_FAIL(hipMemcpy(out_relaxed, ib.out_relaxed, (size_t)it->nq * 4,
                              hipMemcpyDeviceToHost), SPTAG_AMD_ERR_NOGPU);
    return SPTAG_AMD_OK;
}

int sptag_amd_truth(SptagAmdIndex* ix, const void* queries, int32_t nq,
                    int32_t k, int32_t* out_vids, float* out_dists)
{
    if (!ix || !queries || nq <= 0 || k <= 0 || k > MAX_K) return SPTAG_AMD_ERR_PARAM;
    if (!sptag_amd_gpu_available() || !ix->d_vectors) return SPTAG_AMD_ERR_NOGPU;
    std::lock_guard<std::mutex> g(ix->lock);
    HIP_OR_FAIL(hipSetDevice(ix->device), SPTAG_AMD_ERR_NOGPU);

    const size_t n = (size_t)nq * k;
    DevBuf d_q;
    TopkOut out;
    int rc = dev_upload(d_q, queries, (size_t)nq * ix->dim * ix->esz());
    if (rc != SPTAG_AMD_OK) return rc;
    if ((rc = out.ensure(n)) != SPTAG_AMD_OK) return rc;
    if (launch_truth(ix->vt, ix->dm, ix->dev(), d_q.as(), nq, k, out.vids(),
                     out.dists()) != 0)
        return SPTAG_AMD_ERR_NOGPU;
    HIP_OR_FAIL(hipDeviceSynchronize(), SPTAG_AMD_ERR_NOGPU);
    return out.download(out_vids, out_dists, n);
}

/* Host-side distance restatements for the add path's edge arithmetic
 * (RebuildNeighbors / InsertNeighbors recompute pair distances on the
 * host, as the reference does on CPU): same rounding contracts as the
 * kernels/oracle (fused 16-lane order for f32, exact ints for int8). */
static float host_dist(const SptagAmdIndex* ix, const void* a, const void* b)
{
    int d = ix->dim;
    if (ix->vt == VT_INT8) {
        const int8_t* x = (const int8_t*)a;
        const int8_t* y = (const int8_t*)b;
        int32_t s = 0;
        if (ix->dm == DM_L2) {
            for (int i = 0; i < d; i++) { int32_t t = (int32_t)x[i] - y[i]; s += t * t; }
            return (float)s;
        }
        for (int i = 0; i < d; i++) s += (int32_t)x[i] * y[i];
        return (float)(16129 - s);
    }
    const float* x = (const float*)a;
    const float* y = (const float*)b;
    float a16[16], a8[8], a4[4];
    int i = 0, j;
    for (j = 0; j < 16; j++) a16[j] = 0.0f;
    int nd16 = (d >> 4) << 4;
    for (; i < nd16; i += 16)
        for (j = 0; j < 16; j++) {
            float xx = x[i + j], yy = y[i + j];
            a16[j] = ix->dm == DM_L2 ? fmaf(xx - yy, xx - yy, a16[j])
                                     : fmaf(xx, yy, a16[j]);
        }
    for (j = 0; j < 8; j++) a8[j] = a16[j] + a16[j + 8];
    int nd8 = (d >> 3) << 3;
    for (; i < nd8; i += 8)
        for (j = 0; j < 8; j++) {
            float xx = x[i + j], yy = y[i + j];
            a8[j] = ix->dm == DM_L2 ? fmaf(xx - yy, xx - yy, a8[j])
                                    : fmaf(xx, yy, a8[j]);
        }
    for (j = 0; j < 4; j++) a4[j] = a8[j] + a8[j + 4];
    int nd4 = (d >> 2) << 2;
    for (; i < nd4; i += 4)
        for (j = 0; j < 4; j++) {
            float xx = x[i + j], yy = y[i + j];
            a4[j] = ix->dm == DM_L2 ? fmaf(xx - yy, xx - yy, a4[j])
                                    : fmaf(xx, yy, a4[j]);
        }
    float diff = ((a4[0] + a4[1]) + a4[2]) + a4[3];
    for (; i < d; i++) {
        float xx = x[i], yy = y[i];
        diff = ix->dm == DM_L2 ? fmaf(xx - yy, xx - yy, diff) : fmaf(xx, yy, diff);
    }
    return ix->dm == DM_L2 ? diff : 1.0f - diff;
}

static const void* hvec(const SptagAmdIndex* ix, int32_t v)
{
    return ix->h_vectors.data() + (size_t)v * ix->dim * ix->esz();
}

/* RelativeNeighborhoodGraph::RebuildNeighbors (RelativeNeighborhoodGraph.h:18) */
static void host_rebuild_neighbors(SptagAmdIndex* ix, int32_t node,
                                   const int32_t* rv, const float* rd, int nres)
{
    int32_t* nodes = ix->h_graph.data() + (size_t)node * ix->deg;
    int count = 0;
    for (int j = 0; j < nres && count < ix->deg; j++) {
        if (rv[j] < 0) break;
        if (rv[j] == node) continue;
        bool good = true;
        for (int kk = 0; kk < count; kk++) {
            if (host_dist(ix, hvec(ix, nodes[kk]), hvec(ix, rv[j])) < rd[j]) {
                good = false;
                break;
            }
        }
        if (good) nodes[count++] = rv[j];
    }
    for (int j = count; j < ix->deg; j++) nodes[j] = -1;
}

/* RelativeNeighborhoodGraph::InsertNeighbors (RelativeNeighborhoodGraph.h:37) */
static void host_insert_neighbors(SptagAmdIndex* ix, int32_t node,
                                  int32_t insertNode, float insertDist)
{
    int32_t* nodes = ix->h_graph.data() + (size_t)node * ix->deg;
    const void* nodeVec = hvec(ix, node);
    const void* insertVec = hvec(ix, insertNode);
    int checkSize = (nodes[ix->deg - 1] < -1) ? ix->deg - 1 : ix->deg;
    for (int k = 0; k < checkSize; k++) {
        int32_t tmpNode = nodes[k];
        if (tmpNode < 0) { nodes[k] = insertNode; break; }
        const void* tmpVec = hvec(ix, tmpNode);
        float tmpDist = host_dist(ix, tmpVec, nodeVec);
        if (tmpDist > insertDist ||
            (insertDist == tmpDist && insertNode < tmpNode)) {
            nodes[k] = insertNode;
            while (++k < checkSize &&
                   host_dist(ix, tmpVec, nodeVec) <= host_dist(ix, tmpVec, insertVec)) {
                std::swap(tmpNode, nodes[k]);
                if (tmpNode < 0) return;
                tmpVec = hvec(ix, tmpNode);
            }
            break;
        } else if (host_dist(ix, tmpVec, insertVec) < insertDist) {
            break;
        }
    }
}

int sptag_amd_add(SptagAmdIndex* ix, const void* vectors, int32_t nadd,
                  int normalized)
{
    if (!ix || !vectors || nadd <= 0) return SPTAG_AMD_ERR_PARAM;
    if (ix->algo != ALGO_BKT) return SPTAG_AMD_ERR_UNSUPP;
    if (!sptag_amd_gpu_available() || !ix->d_vectors) {
        fprintf(stderr, "sptag_amd: add requires a HIP device (refine searches)\n");
        return SPTAG_AMD_ERR_NOGPU;
    }
    std::lock_guard<std::mutex> g(ix->lock);
    HIP_OR_FAIL(hipSetDevice(ix->device), SPTAG_AMD_ERR_NOGPU);

    int32_t begin = ix->n, end = ix->n + nadd;
    size_t esz = ix->esz();
    /* host copies (AddIndex: m_pSamples/m_pGraph/m_deletedID AddBatch) */
    ix->h_vectors.resize((size_t)end * ix->dim * esz);
    memcpy(ix->h_vectors.data() + (size_t)begin * ix->dim * esz, vectors,
           (size_t)nadd * ix->dim * esz);
    ix->h_graph.resize((size_t)end * ix->deg, -1);
    if (!ix->h_deleted.empty()) ix->h_deleted.resize((size_t)end, 0);
    ix->n = end;

    if (ix->dm == DM_COSINE && !normalized) {
        /* Utils::Normalize to norm=base, C-cast truncation for int8
         * (CommonUtils.h:62) */
        for (int32_t i = begin; i < end; i++) {
            char* vp = ix->h_vectors.data() + (size_t)i * ix->dim * esz;
            double s = 0;
            if (ix->vt == VT_FLOAT) {
                float* v = (float*)vp;
                for (int d = 0; d < ix->dim; d++) s += (double)v[d] * v[d];
                s = sqrt(s);
                if (s > 0) for (int d = 0; d < ix->dim; d++) v[d] = (float)(v[d] / s);
            } else {
                int8_t* v = (int8_t*)vp;
                for (int d = 0; d < ix->dim; d++) s += (double)v[d] * v[d];
                s = sqrt(s);
                if (s > 0) for (int d = 0; d < ix->dim; d++)
                    v[d] = (int8_t)(v[d] * 127.0 / s);
            }
        }
    }

    /* device: re-allocate vectors+graph at the new size; the handle keeps
     * its old arrays until both uploads have succeeded */
    DevBuf nv, ng;
    int rc = dev_upload(nv, ix->h_vectors.data(), ix->h_vectors.size());
    if (rc == SPTAG_AMD_OK)
        rc = dev_upload(ng, ix->h_graph.data(), ix->h_graph.size() * 4);
    if (rc != SPTAG_AMD_OK) return rc;
    ix->d_vectors = std::move(nv);
    ix->d_graph = std::move(ng);
    if (ix->has_deleted) {
        rc = dev_upload(ix->d_deleted, ix->h_deleted.data(), ix->h_deleted.size());
        if (rc != SPTAG_AMD_OK) return rc;
    }

    /* per new node: RefineNode (search CEF+1 at MaxCheckForRefineGraph with
     * the refine dispatch flags, then RNG rebuild + two-way inserts).
     * Sequential, as the reference's add loop is (BKTIndex.cpp:966-969);
     * each refine sees the edges of previously added nodes. */
    const int k = 500 + 1;   /* AddCEF default (ParameterDefinitionList) */
    std::vector<int32_t> rv(k);
    std::vector<float> rd(k);
    /* d_rows/d_rowidx stage the batched changed-row upload: one H2D + one
     * scatter per added node instead of one 128 B hipMemcpy per touched
     * edge (the round-1 form did up to ~500 tiny copies per add). */
    TopkOut out;
    DevBuf d_q, d_rows, d_rowidx;
    if ((rc = out.ensure(k)) != SPTAG_AMD_OK) return rc;
    HIP_OR_FAIL(d_q.alloc((size_t)ix->dim * esz), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(d_rows.alloc((size_t)(k + 1) * ix->deg * 4), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(d_rowidx.alloc((size_t)(k + 1) * 4), SPTAG_AMD_ERR_OOM);
    std::vector<int32_t> hrows((size_t)(k + 1) * ix->deg);
    std::vector<int32_t> hidx(k + 1);
    for (int32_t node = begin; node < end; node++) {
        HIP_OR_FAIL(hipMemcpy(d_q.as(), hvec(ix, node), (size_t)ix->dim * esz,
                              hipMemcpyHostToDevice), SPTAG_AMD_ERR_NOGPU);
        rc = search_device_core(ix, d_q.as(), 1, k, 8192 /*MaxCheckForRefineGraph*/,
                                out.vids(), out.dists(), true);
        if (rc != SPTAG_AMD_OK) return rc;
        if ((rc = out.download(rv.data(), rd.data(), k)) != SPTAG_AMD_OK) return rc;
        host_rebuild_neighbors(ix, node, rv.data(), rd.data(), k);
        int nrows = 0;
        hidx[nrows++] = node;
        for (int j = 0; j < k; j++) {
            if (rv[j] < 0) break;
            if (rv[j] == node) continue;
            host_insert_neighbors(ix, rv[j], node, rd[j]);
            hidx[nrows++] = rv[j];
        }
        /* dedup row ids, stage payloads, one H2D + one scatter */
        std::sort(hidx.begin(), hidx.begin() + nrows);
        nrows = (int)(std::unique(hidx.begin(), hidx.begin() + nrows) -
                      hidx.begin());
        for (int j = 0; j < nrows; j++)
            memcpy(&hrows[(size_t)j * ix->deg],
                   ix->h_graph.data() + (size_t)hidx[j] * ix->deg,
                   (size_t)ix->deg * 4);
        HIP_OR_FAIL(hipMemcpy(d_rows.as(), hrows.data(), (size_t)nrows * ix->deg * 4,
                              hipMemcpyHostToDevice), SPTAG_AMD_ERR_NOGPU);
        HIP_OR_FAIL(hipMemcpy(d_rowidx.as(), hidx.data(), (size_t)nrows * 4,
                              hipMemcpyHostToDevice), SPTAG_AMD_ERR_NOGPU);
        launch_copy_rows(false, ix->d_graph.as(), d_rows.as(), ix->deg * 4,
                         d_rowidx.as<int32_t>(), nrows);
        HIP_OR_FAIL(hipDeviceSynchronize(), SPTAG_AMD_ERR_NOGPU);
    }
    return SPTAG_AMD_OK;
}

int sptag_amd_delete_by_vector(SptagAmdIndex* ix, const void* vectors,
                               int32_t n)
{
    /* reference DeleteIndex(const void*, SizeType) (BKTIndex.cpp:876-891):
     * search CEF=1000 results per vector, delete every id at distance
     * < 1e-6 (exact duplicates of the given vector). */
    if (!ix || !vectors || n <= 0) return SPTAG_AMD_ERR_PARAM;
    if (ix->algo != ALGO_BKT) return SPTAG_AMD_ERR_UNSUPP;
    if (!sptag_amd_gpu_available() || !ix->d_vectors) return SPTAG_AMD_ERR_NOGPU;
    const int k = 1000;   /* m_iCEF default */
    std::vector<int32_t> rv((size_t)n * k);
    std::vector<float> rd((size_t)n * k);
    int rc = sptag_amd_search_batch(ix, vectors, n, k, 0, rv.data(), rd.data());
    if (rc != SPTAG_AMD_OK) return rc;
    std::vector<int32_t> dels;
    for (int32_t i = 0; i < n; i++)
        for (int j = 0; j < k; j++) {
            if (rv[(size_t)i * k + j] < 0) break;
            if (rd[(size_t)i * k + j] < 1e-6f) dels.push_back(rv[(size_t)i * k + j]);
        }
    if (dels.empty()) return SPTAG_AMD_OK;
    return sptag_amd_delete(ix, dels.data(), (int32_t)dels.size());
}

int sptag_amd_delete(SptagAmdIndex* ix, const int32_t* vids, int32_t n)
{
    if (!ix || !vids || n <= 0) return SPTAG_AMD_ERR_PARAM;
    std::lock_guard<std::mutex> g(ix->lock);
    if (ix->h_deleted.empty()) ix->h_deleted.assign((size_t)ix->n, 0);
    for (int32_t i = 0; i < n; i++) {
        int32_t v = vids[i];
        if (v < 0 || v >= ix->n) return SPTAG_AMD_ERR_PARAM;
        if (!ix->h_deleted[v]) {
            ix->h_deleted[v] = 1;
            ix->deleted_count++;
        }
    }
    ix->has_deleted = ix->deleted_count > 0;
    if (sptag_amd_gpu_available() && ix->d_vectors) {
        HIP_OR_FAIL(hipSetDevice(ix->device), SPTAG_AMD_ERR_NOGPU);
        HIP_OR_FAIL(ix->d_deleted.ensure(ix->h_deleted.size()), SPTAG_AMD_ERR_OOM);
        HIP_OR_FAIL(hipMemcpy(ix->d_deleted.as(), ix->h_deleted.data(),
                              ix->h_deleted.size(), hipMemcpyHostToDevice),
                    SPTAG_AMD_ERR_NOGPU);
    }
    return SPTAG_AMD_OK;
}

int64_t sptag_amd_deleted_count(const SptagAmdIndex* ix)
{
    return ix ? ix->deleted_count : -1;
}

int sptag_amd_save_index(SptagAmdIndex* ix, const char* folder)
{
    if (!ix || !folder) return SPTAG_AMD_ERR_PARAM;
    std::string dir(folder);
    if (!dir.empty() && dir.back() != '/') dir += '/';

    int32_t vh[2] = {ix->n, ix->dim};
    if (!write_file(dir + "vectors.bin",
                    {{vh, 8}, {ix->h_vectors.data(), ix->h_vectors.size()}}))
        return SPTAG_AMD_ERR_IO;
    const size_t node_bytes = ix->algo == ALGO_KDT ? 16 : 12;
    if (!write_file(dir + "tree.bin",
                    {{&ix->ntrees, 4},
                     {ix->h_tree_start.data(), (size_t)ix->ntrees * 4},
                     {&ix->n_tree_nodes, 4},
                     {ix->h_tree.data(), (size_t)ix->n_tree_nodes * node_bytes}}))
        return SPTAG_AMD_ERR_IO;
    int32_t gh[2] = {ix->n, ix->deg};
    if (!write_file(dir + "graph.bin",
                    {{gh, 8}, {ix->h_graph.data(), ix->h_graph.size() * 4}}))
        return SPTAG_AMD_ERR_IO;
    {
        std::vector<uint8_t> del = ix->h_deleted;
        if (del.empty()) del.assign((size_t)ix->n, 0);
        int32_t dh[3] = {(int32_t)ix->deleted_count, ix->n, 1};
        if (!write_file(dir + "deletes.bin", {{dh, 12}, {del.data(), del.size()}}))
            return SPTAG_AMD_ERR_IO;
    }
    {
        FILE* f = fopen((dir + "indexloader.ini").c_str(), "wb");
        if (!f) return SPTAG_AMD_ERR_IO;
        if (ix->algo == ALGO_KDT) {
            fprintf(f,
                    "[Index]\nIndexAlgoType=KDT\nValueType=%s\n\n"
                    "TreeFilePath=tree.bin\nGraphFilePath=graph.bin\n"
                    "VectorFilePath=vectors.bin\nDeleteVectorFilePath=deletes.bin\n"
                    "KDTNumber=%d\nNumTopDimensionKDTSplit=5\nSamples=100\n"
                    "TPTNumber=32\nTPTLeafSize=2000\nNumTopDimensionTPTSplit=5\n"
                    "NeighborhoodSize=%d\nGraphNeighborhoodScale=2.000000\n"
                    "GraphCEFScale=2.000000\nRefineIterations=2\nCEF=1000\n"
                    "MaxCheckForRefineGraph=8192\nNumberOfThreads=4\n"
                    "DistCalcMethod=%s\nMaxCheck=%d\n"
                    "ThresholdOfNumberOfContinuousNoBetterPropagation=%d\n"
                    "NumberOfInitialDynamicPivots=%d\n"
                    "NumberOfOtherDynamicPivots=%d\nHashTableExponent=2\n"
                    "DataBlockSize=1048576\nDataCapacity=2147483647\n"
                    "MetaRecordSize=10\n",
                    ix->vt == VT_FLOAT ? "Float" : "Int8", ix->ntrees, ix->deg,
                    ix->dm == DM_L2 ? "L2" : "Cosine", ix->default_maxcheck,
                    ix->nobetter_threshold, ix->init_pivots, ix->other_pivots);
            fclose(f);
            return SPTAG_AMD_OK;
        }
        fprintf(f,
                "[Index]\n"
                "IndexAlgoType=BKT\n"
                "ValueType=%s\n\n"
                "TreeFilePath=tree.bin\nGraphFilePath=graph.bin\n"
                "VectorFilePath=vectors.bin\nDeleteVectorFilePath=deletes.bin\n"
                "EnableBfs=0\nBKTNumber=%d\nBKTKmeansK=32\nBKTLeafSize=8\n"
                "Samples=1000\nBKTLambdaFactor=100.000000\nTPTNumber=32\n"
                "TPTLeafSize=2000\nNumTopDimensionTpTreeSplit=5\n"
                "NeighborhoodSize=%d\nGraphNeighborhoodScale=2.000000\n"
                "GraphCEFScale=2.000000\nRefineIterations=2\nEnableRebuild=0\n"
                "CEF=1000\nAddCEF=500\nMaxCheckForRefineGraph=8192\n"
                "RNGFactor=1.000000\nGPUGraphType=2\nGPURefineSteps=0\n"
                "GPURefineDepth=30\nGPULeafSize=500\nHeadNumGPUs=1\n"
                "TPTBalanceFactor=2\nNumberOfThreads=4\nDistCalcMethod=%s\n"
                "DeletePercentageForRefine=0.400000\nAddCountForRebuild=1000\n"
                "MaxCheck=%d\n"
                "ThresholdOfNumberOfContinuousNoBetterPropagation=3\n"
                "NumberOfInitialDynamicPivots=%d\nNumberOfOtherDynamicPivots=%d\n"
                "HashTableExponent=2\nDataBlockSize=1048576\n"
                "DataCapacity=2147483647\nMetaRecordSize=10\n",
                ix->vt == VT_FLOAT ? "Float" : "Int8", ix->ntrees, ix->deg,
                ix->dm == DM_L2 ? "L2" : "Cosine", ix->default_maxcheck,
                ix->init_pivots, ix->other_pivots);
        fclose(f);
    }
    return SPTAG_AMD_OK;
}

int32_t sptag_amd_num_vectors(const SptagAmdIndex* ix) { return ix ? ix->n : -1; }
int32_t sptag_amd_dim(const SptagAmdIndex* ix) { return ix ? ix->dim : -1; }
int sptag_amd_valuetype(const SptagAmdIndex* ix) { return ix ? ix->vt : -1; }
int sptag_amd_distmethod(const SptagAmdIndex* ix) { return ix ? ix->dm : -1; }
int32_t sptag_amd_degree(const SptagAmdIndex* ix) { return ix ? ix->deg : -1; }
int32_t sptag_amd_default_maxcheck(const SptagAmdIndex* ix)
{ return ix ? ix->default_maxcheck : -1; }
int sptag_amd_algo(const SptagAmdIndex* ix) { return ix ? ix->algo : -1; }

void sptag_amd_set_search_params(SptagAmdIndex* ix, int32_t init_pivots,
                                 int32_t other_pivots,
                                 int32_t nobetter_threshold,
                                 int32_t default_maxcheck)
{
    if (!ix) return;
    std::lock_guard<std::mutex> g(ix->lock);   /* a search may be in flight */
    if (init_pivots > 0) ix->init_pivots = init_pivots;
    if (other_pivots > 0) ix->other_pivots = other_pivots;
    if (nobetter_threshold > 0) ix->nobetter_threshold = nobetter_threshold;
    if (default_maxcheck > 0) ix->default_maxcheck = default_maxcheck;
}

}  /* extern "C" */

/* ------------------------------------------------------------------ *
 * shard sets: several indexes searched as one, merged on the GPU
 * (reference AggregatorService::AggregateResults,
 * src/Aggregator/AggregatorService.cpp:363)
 * ------------------------------------------------------------------ */

/* the shards of one device, and what the set keeps there for them */
struct ShardGroup {
    int device = 0;
    std::vector<int> ids;   /* shard numbers, ascending */
    DevBuf d_q;             /* the query batch, on devices other than shard 0's */
    DevBuf d_v, d_d;        /* these shards' lists, likewise: [ids.size()][nq][k] */
};

struct SptagAmdShards {
    std::vector<SptagAmdIndex*> shards;   /* not owned */
    MergeBases bases;
    std::vector<ShardGroup> groups;       /* groups[0] holds shard 0 */
    std::mutex lock;                      /* the buffers below serve one call at a time */
    DevBuf d_allv, d_alld;                /* [S][nq][k] on the device of shard 0 */
};

/* Run fn(group) for every device group: in the calling thread when all
 * shards share a device, else one thread per device, each of which selects
 * its device first. Returns the first group's error, in group order. */
template <class F>
static int for_each_group(SptagAmdShards* set, F&& fn)
{
    std::vector<int> rc(set->groups.size(), SPTAG_AMD_OK);
    auto run = [&](size_t g) {
        if (hipSetDevice(set->groups[g].device) != hipSuccess) {
            rc[g] = SPTAG_AMD_ERR_NOGPU;
            return;
        }
        rc[g] = fn(set->groups[g]);
    };
    if (set->groups.size() == 1) {
        run(0);
    } else {
        std::vector<std::thread> th;
        for (size_t g = 0; g < set->groups.size(); g++) th.emplace_back(run, g);
        for (auto& t : th) t.join();
    }
    for (int r : rc)
        if (r != SPTAG_AMD_OK) return r;
    return SPTAG_AMD_OK;
}

static int check_shards_args(SptagAmdShards* set, const void* q, int32_t nq, int32_t k)
{
    if (!set || !q || nq <= 0 || k <= 0 || k > MAX_K) return SPTAG_AMD_ERR_PARAM;
    bool resident = sptag_amd_gpu_available();
    for (SptagAmdIndex* ix : set->shards) resident = resident && ix->d_vectors;
    if (!resident) {
        fprintf(stderr,
                "sptag_amd: shard search requires a HIP device (%s); no CPU fallback\n",
                sptag_amd_build_info());
        return SPTAG_AMD_ERR_NOGPU;
    }
    return SPTAG_AMD_OK;
}

static int merge_args_ok(int32_t nshards, int32_t nq, int32_t k_in, int32_t k_out,
                         const void* vids, const void* dists, const int32_t* vid_base,
                         const void* out_vids, const void* out_dists)
{
    if (nshards < 1 || nshards > MAX_SHARDS || nq <= 0 || k_in <= 0 || k_in > MAX_K ||
        k_out <= 0 || k_out > MAX_K || !vids || !dists || !vid_base || !out_vids ||
        !out_dists)
        return SPTAG_AMD_ERR_PARAM;
    for (int32_t s = 0; s < nshards; s++)
        if (vid_base[s] < 0) return SPTAG_AMD_ERR_PARAM;
    if (!sptag_amd_gpu_available()) {
        fprintf(stderr, "sptag_amd: merge_topk requires a HIP device\n");
        return SPTAG_AMD_ERR_NOGPU;
    }
    return SPTAG_AMD_OK;
}

/* merge on the current device; returns once the output is complete */
static int merge_on_device(const MergeBases& bases, int32_t nshards, int32_t nq,
                           int32_t k_in, int32_t k_out, const int32_t* d_vids,
                           const float* d_dists, int32_t* d_out_vids, float* d_out_dists)
{
    int err = launch_merge_topk(d_vids, d_dists, bases, nshards, nq, k_in, k_out,
                                d_out_vids, d_out_dists);
    if (err != 0) {
        fprintf(stderr, "sptag_amd: merge launch failed %d\n", err);
        return SPTAG_AMD_ERR_INTERNAL;
    }
    HIP_OR_FAIL(hipDeviceSynchronize(), SPTAG_AMD_ERR_NOGPU);
    return SPTAG_AMD_OK;
}

/* Search every shard into set->d_allv/d_alld ([S][nq][k] on the device of
 * shard 0, the current device on return). d_q is on that device. */
static int shards_fan_out_search(SptagAmdShards* set, const void* d_q, int32_t nq,
                                 int32_t k, int32_t max_check)
{
    const int S = (int)set->shards.size();
    const int dev0 = set->groups[0].device;
    const size_t list = (size_t)nq * k;          /* entries of one shard's lists */
    const size_t qbytes = (size_t)nq * set->shards[0]->dim * set->shards[0]->esz();
    HIP_OR_FAIL(hipSetDevice(dev0), SPTAG_AMD_ERR_NOGPU);
    HIP_OR_FAIL(set->d_allv.ensure((size_t)S * list * 4), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(set->d_alld.ensure((size_t)S * list * 4), SPTAG_AMD_ERR_OOM);
    int32_t* allv = set->d_allv.as<int32_t>();
    float* alld = set->d_alld.as<float>();

    int rc = for_each_group(set, [&](ShardGroup& g) -> int {
        const bool home = g.device == dev0;
        const void* q = d_q;
        if (!home) {
            HIP_OR_FAIL(g.d_q.ensure(qbytes), SPTAG_AMD_ERR_OOM);
            HIP_OR_FAIL(g.d_v.ensure(g.ids.size() * list * 4), SPTAG_AMD_ERR_OOM);
            HIP_OR_FAIL(g.d_d.ensure(g.ids.size() * list * 4), SPTAG_AMD_ERR_OOM);
            HIP_OR_FAIL(hipMemcpyPeer(g.d_q.as(), g.device, d_q, dev0, qbytes),
                        SPTAG_AMD_ERR_NOGPU);
            q = g.d_q.as();
        }
        for (size_t j = 0; j < g.ids.size(); j++) {
            const int s = g.ids[j];
            SptagAmdIndex* ix = set->shards[s];
            int32_t* v = home ? allv + s * list : g.d_v.as<int32_t>() + j * list;
            float* d = home ? alld + s * list : g.d_d.as<float>() + j * list;
            int r;
            {
                std::lock_guard<std::mutex> lk(ix->lock);
                r = search_device_core(ix, q, nq, k, max_check, v, d);
            }
            if (r != SPTAG_AMD_OK) return r;
            if (!home) {
                /* staged through the host where the devices are not peers */
                HIP_OR_FAIL(hipMemcpyPeer(allv + s * list, dev0, v, g.device, list * 4),
                            SPTAG_AMD_ERR_NOGPU);
                HIP_OR_FAIL(hipMemcpyPeer(alld + s * list, dev0, d, g.device, list * 4),
                            SPTAG_AMD_ERR_NOGPU);
            }
        }
        return SPTAG_AMD_OK;
    });
    HIP_OR_FAIL(hipSetDevice(dev0), SPTAG_AMD_ERR_NOGPU);
    return rc;
}

extern "C" {

int sptag_amd_merge_topk_device(int device, int32_t nshards, int32_t nq, int32_t k_in,
                                int32_t k_out, const int32_t* d_vids,
                                const float* d_dists, const int32_t* vid_base,
                                int32_t* d_out_vids, float* d_out_dists)
{
    int rc = merge_args_ok(nshards, nq, k_in, k_out, d_vids, d_dists, vid_base,
                           d_out_vids, d_out_dists);
    if (rc != SPTAG_AMD_OK) return rc;
    MergeBases bases = {};
    std::copy(vid_base, vid_base + nshards, bases.b);
    HIP_OR_FAIL(hipSetDevice(device), SPTAG_AMD_ERR_NOGPU);
    return merge_on_device(bases, nshards, nq, k_in, k_out, d_vids, d_dists,
                           d_out_vids, d_out_dists);
}

int sptag_amd_merge_topk(int device, int32_t nshards, int32_t nq, int32_t k_in,
                         int32_t k_out, const int32_t* vids, const float* dists,
                         const int32_t* vid_base, int32_t* out_vids, float* out_dists)
{
    int rc = merge_args_ok(nshards, nq, k_in, k_out, vids, dists, vid_base, out_vids,
                           out_dists);
    if (rc != SPTAG_AMD_OK) return rc;
    HIP_OR_FAIL(hipSetDevice(device), SPTAG_AMD_ERR_NOGPU);
    const size_t ibytes = (size_t)nshards * nq * k_in * 4, n = (size_t)nq * k_out;
    DevBuf d_v, d_d;
    TopkOut out;
    if ((rc = dev_upload(d_v, vids, ibytes)) != SPTAG_AMD_OK) return rc;
    if ((rc = dev_upload(d_d, dists, ibytes)) != SPTAG_AMD_OK) return rc;
    if ((rc = out.ensure(n)) != SPTAG_AMD_OK) return rc;
    rc = sptag_amd_merge_topk_device(device, nshards, nq, k_in, k_out,
                                     d_v.as<int32_t>(), d_d.as<float>(), vid_base,
                                     out.vids(), out.dists());
    return rc != SPTAG_AMD_OK ? rc : out.download(out_vids, out_dists, n);
}

SptagAmdShards* sptag_amd_shards_create(SptagAmdIndex* const* shards, int32_t nshards,
                                        const int32_t* vid_base)
{
    if (nshards < 1 || nshards > MAX_SHARDS || !shards) {
        fprintf(stderr, "sptag_amd: a shard set holds 1..%d shards, got %d\n",
                (int)MAX_SHARDS, nshards);
        return nullptr;
    }
    std::unique_ptr<SptagAmdShards> set(new SptagAmdShards());
    set->bases = MergeBases{};
    int64_t next = 0;   /* running sum of num_vectors */
    for (int32_t s = 0; s < nshards; s++) {
        const SptagAmdIndex* ix = shards[s];
        if (!ix) {
            fprintf(stderr, "sptag_amd: shard %d is NULL\n", s);
            return nullptr;
        }
        const SptagAmdIndex* first = shards[0];
        if (ix->dim != first->dim || ix->vt != first->vt || ix->dm != first->dm) {
            fprintf(stderr, "sptag_amd: shard %d differs from shard 0 in dim, value "
                            "type or distance method\n", s);
            return nullptr;
        }
        const int64_t base = vid_base ? vid_base[s] : next;
        if (base < 0 || base + ix->n > (int64_t)INT32_MAX) {
            fprintf(stderr, "sptag_amd: shard %d: base %lld + %d vectors does not fit "
                            "int32\n", s, (long long)base, ix->n);
            return nullptr;
        }
        set->bases.b[s] = (int32_t)base;
        next = base + ix->n;
        set->shards.push_back(shards[s]);
        /* shard 0 opens group 0, so that is the merge device's group */
        auto g = std::find_if(set->groups.begin(), set->groups.end(),
                              [&](const ShardGroup& x) { return x.device == ix->device; });
        if (g == set->groups.end()) {
            set->groups.emplace_back();
            g = set->groups.end() - 1;
            g->device = ix->device;
        }
        g->ids.push_back(s);
    }
    return set.release();
}

void sptag_amd_shards_free(SptagAmdShards* set)
{
    if (set) delete set;   /* the set's own buffers only; the shards stay */
}

int32_t sptag_amd_shards_count(const SptagAmdShards* set)
{
    return set ? (int32_t)set->shards.size() : -1;
}

int64_t sptag_amd_shards_num_vectors(const SptagAmdShards* set)
{
    if (!set) return -1;
    int64_t n = 0;
    for (const SptagAmdIndex* ix : set->shards) n += ix->n;
    return n;
}

int sptag_amd_shards_search_batch_device(SptagAmdShards* set, const void* d_queries,
                                         int32_t nq, int32_t k, int32_t max_check,
                                         int32_t* d_out_vids, float* d_out_dists)
{
    int rc = check_shards_args(set, d_queries, nq, k);
    if (rc != SPTAG_AMD_OK) return rc;
    if (!d_out_vids || !d_out_dists) return SPTAG_AMD_ERR_PARAM;
    std::lock_guard<std::mutex> g(set->lock);
    rc = shards_fan_out_search(set, d_queries, nq, k, max_check);
    if (rc != SPTAG_AMD_OK) return rc;
    return merge_on_device(set->bases, (int32_t)set->shards.size(), nq, k, k,
                           set->d_allv.as<int32_t>(), set->d_alld.as<float>(),
                           d_out_vids, d_out_dists);
}

int sptag_amd_shards_search_batch(SptagAmdShards* set, const void* queries, int32_t nq,
                                  int32_t k, int32_t max_check, int32_t* out_vids,
                                  float* out_dists)
{
    int rc = check_shards_args(set, queries, nq, k);
    if (rc != SPTAG_AMD_OK) return rc;
    if (!out_vids || !out_dists) return SPTAG_AMD_ERR_PARAM;
    HIP_OR_FAIL(hipSetDevice(set->groups[0].device), SPTAG_AMD_ERR_NOGPU);
    const SptagAmdIndex* ix0 = set->shards[0];
    const size_t qbytes = (size_t)nq * ix0->dim * ix0->esz(), n = (size_t)nq * k;
    DevBuf d_q;
    TopkOut out;
    if ((rc = dev_upload(d_q, queries, qbytes)) != SPTAG_AMD_OK) return rc;
    if ((rc = out.ensure(n)) != SPTAG_AMD_OK) return rc;
    rc = sptag_amd_shards_search_batch_device(set, d_q.as(), nq, k, max_check,
                                              out.vids(), out.dists());
    return rc != SPTAG_AMD_OK ? rc : out.download(out_vids, out_dists, n);
}

int sptag_amd_shards_truth(SptagAmdShards* set, const void* queries, int32_t nq,
                           int32_t k, int32_t* out_vids, float* out_dists)
{
    int rc = check_shards_args(set, queries, nq, k);
    if (rc != SPTAG_AMD_OK) return rc;
    if (!out_vids || !out_dists) return SPTAG_AMD_ERR_PARAM;
    const int S = (int)set->shards.size();
    const size_t list = (size_t)nq * k;
    std::vector<int32_t> hv((size_t)S * list);
    std::vector<float> hd((size_t)S * list);
    rc = for_each_group(set, [&](ShardGroup& g) -> int {
        for (int s : g.ids) {
            int r = sptag_amd_truth(set->shards[s], queries, nq, k,
                                    hv.data() + s * list, hd.data() + s * list);
            if (r != SPTAG_AMD_OK) return r;
        }
        return SPTAG_AMD_OK;
    });
    if (rc != SPTAG_AMD_OK) return rc;
    return sptag_amd_merge_topk(set->groups[0].device, S, nq, k, k, hv.data(),
                                hd.data(), set->bases.b, out_vids, out_dists);
}

}  /* extern "C" */

/* heap probe (common.h): upload the script, run both forms, download */
extern "C" int sptagamd_dbg_heap_probe(int device, int32_t cap, int32_t ref_cap, int32_t lsplit,
                            int32_t nops, const int32_t* ops, const int32_t* nodes,
                            const float* dists, void* out_heaps, void* out_pops,
                            int32_t* out_final)
{
    using namespace sptag_amd;
    if (!ops || !nodes || !dists || !out_heaps || !out_pops || !out_final ||
        cap < 1 || cap > HEAP_PROBE_MAX_CAP || ref_cap < cap || lsplit < 0 ||
        lsplit > HEAP_PROBE_MAX_LSPLIT || nops < 1)
        return SPTAG_AMD_ERR_PARAM;
    if (!sptag_amd_gpu_available()) return SPTAG_AMD_ERR_NOGPU;
    HIP_OR_FAIL(hipSetDevice(device), SPTAG_AMD_ERR_NOGPU);
    const size_t hbytes = 2 * ((size_t)cap + 1) * 8, pbytes = 2 * (size_t)nops * 8;
    DevBuf d_ops, d_nodes, d_dists, d_heaps, d_pops, d_final;
    int rc;
    if ((rc = dev_upload(d_ops, ops, (size_t)nops * 4)) != SPTAG_AMD_OK) return rc;
    if ((rc = dev_upload(d_nodes, nodes, (size_t)nops * 4)) != SPTAG_AMD_OK) return rc;
    if ((rc = dev_upload(d_dists, dists, (size_t)nops * 4)) != SPTAG_AMD_OK) return rc;
    HIP_OR_FAIL(d_heaps.alloc(hbytes), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(d_pops.alloc(pbytes), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(d_final.alloc(16), SPTAG_AMD_ERR_OOM);
    HIP_OR_FAIL(hipMemset(d_heaps.as(), 0xff, hbytes), SPTAG_AMD_ERR_NOGPU);
    HIP_OR_FAIL(hipMemset(d_pops.as(), 0xff, pbytes), SPTAG_AMD_ERR_NOGPU);
    HIP_OR_FAIL(hipMemset(d_final.as(), 0, 16), SPTAG_AMD_ERR_NOGPU);
    HeapProbeArgs a{cap, ref_cap, lsplit, nops, d_ops.as<int32_t>(),
                    d_nodes.as<int32_t>(), d_dists.as<float>(), d_heaps.as(),
                    d_pops.as(), d_final.as<int32_t>()};
    if (launch_heap_probe(a) != 0) return SPTAG_AMD_ERR_INTERNAL;
    HIP_OR_FAIL(hipDeviceSynchronize(), SPTAG_AMD_ERR_NOGPU);
    HIP_OR_FAIL(hipMemcpy(out_heaps, d_heaps.as(), hbytes, hipMemcpyDeviceToHost),
                SPTAG_AMD_ERR_NOGPU);
    HIP_OR_FAIL(hipMemcpy(out_pops, d_pops.as(), pbytes, hipMemcpyDeviceToHost),
                SPTAG_AMD_ERR_NOGPU);
    HIP_OR_FAIL(hipMemcpy(out_final, d_final.as(), 16, hipMemcpyDeviceToHost),
                SPTAG_AMD_ERR_NOGPU);
    return SPTAG_AMD_OK;
}
