// ulg_ctx.cpp -- context lifecycle, errors, profiling for libulg.so.
#include <atomic>
#include <mutex>
#include <cstdio>
#include <cstring>

#include "disc_bdeu.h"  // kBdeuEssMin, kBdeuEssMax
#include "search_internal.h"

namespace ulg {

int set_err(ulg_ctx *c, int code, const std::string &msg) {
    if (c) {
        // the wide scoring layers run one host thread per stream group
        std::lock_guard<std::mutex> lk(c->mu);
        c->err = msg;
    }
    return code;
}

const std::vector<uint32_t> &host_binom() {
    static std::vector<uint32_t> t = [] {
        std::vector<uint32_t> b(64 * kBinomK, 0);
        for (int a = 0; a < 64; ++a)
            for (int k = 0; k < kBinomK; ++k) {
                uint64_t v = binom64(a, k);
                b[a * kBinomK + k] = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
            }
        return b;
    }();
    return t;
}

const std::vector<uint64_t> &host_binom64() {
    static std::vector<uint64_t> t = [] {
        std::vector<uint64_t> b(64 * 64, 0);
        for (int a = 0; a < 64; ++a)
            for (int k = 0; k < 64; ++k) b[a * 64 + k] = binom64(a, k);
        return b;
    }();
    return t;
}

void prof_begin(ulg_ctx *c, const char *name) { prof_begin_s(c, name, c->stream); }
void prof_end(ulg_ctx *c) { prof_end_s(c, c->stream); }

// The record a thread's prof_end_s closes: its own last prof_begin_s (the
// wide scoring layers drive their stream groups from several host threads).
thread_local int64_t t_prof_rec = -1;

void prof_begin_s(ulg_ctx *c, const char *name, hipStream_t stream) {
    t_prof_rec = -1;
    if (!c->prof || (!c->prof_only.empty() && !c->prof_only.count(name))) return;
    std::lock_guard<std::mutex> lk(c->mu);
    ProfRec r;
    r.name = name;
    // events come from a per-context pool: creating two per kernel costs more
    // than the small layers' kernels themselves
    for (hipEvent_t *e : {&r.start, &r.stop}) {
        if (!c->event_pool.empty()) {
            *e = c->event_pool.back();
            c->event_pool.pop_back();
        } else {
            (void)hipEventCreate(e);
        }
    }
    (void)hipEventRecord(r.start, stream);
    t_prof_rec = (int64_t)c->pending.size();
    c->pending.push_back(r);
}

void prof_end_s(ulg_ctx *c, hipStream_t stream) {
    if (t_prof_rec < 0) return;
    std::lock_guard<std::mutex> lk(c->mu);
    if (t_prof_rec < (int64_t)c->pending.size()) (void)hipEventRecord(c->pending[(size_t)t_prof_rec].stop, stream);
    t_prof_rec = -1;
}

void prof_collect(ulg_ctx *c) {
    for (auto &r : c->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(r.stop) == hipSuccess && hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess)
            c->prof_ms[r.name].push_back(ms);
        if (r.graph) continue;  // the graph records these again on every replay
        c->event_pool.push_back(r.start);
        c->event_pool.push_back(r.stop);
    }
    c->pending.clear();
}

void graph_reset(ulg_ctx *c) {
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    if (c->gexec) (void)hipGraphExecDestroy(c->gexec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    c->gexec = nullptr;
    c->graph = nullptr;
    c->gkey.clear();
    for (const ProfRec &r : c->gprof) {
        c->event_pool.push_back(r.start);
        c->event_pool.push_back(r.stop);
    }
    c->gprof.clear();
}

// ---- dev_buf.h's memory, over HIP ----------------------------------------------
// bytes live through DevBuf / PinnedBuf in this process (ulg_get_info)
static std::atomic<int64_t> g_device_bytes{0}, g_pinned_bytes{0};

int dev_alloc(void **p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) g_device_bytes += (int64_t)bytes;
    return (int)e;
}
int dev_free(void *p, size_t bytes) {
    g_device_bytes -= (int64_t)bytes;
    return (int)hipFree(p);
}
int pinned_alloc(void **p, size_t bytes) {
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) g_pinned_bytes += (int64_t)bytes;
    return (int)e;
}
int pinned_free(void *p, size_t bytes) {
    g_pinned_bytes -= (int64_t)bytes;
    return (int)hipHostFree(p);
}
int alloc_failed(ulg_ctx *c, const char *call, int status) {
    return set_err(c, ULG_ERR_HIP, std::string(call) + " failed: " + hipGetErrorString((hipError_t)status));
}
int dev_upload(ulg_ctx *c, void *dst, const void *src, size_t bytes) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return set_err(c, ULG_ERR_HIP, std::string("hipMemcpyAsync failed: ") + hipGetErrorString(e));
    return ULG_OK;
}

CtxStreams::~CtxStreams() {
    for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
    for (hipStream_t s : aux_streams) (void)hipStreamDestroy(s);
    for (hipEvent_t e : sync_events) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
}

}  // namespace ulg

// The one place the teardown order is written.  With the context's device
// current: wait until the stream is idle, so that no launch still reads a
// buffer; drop the captured graph, which hands its events back to the pool;
// delete the search and .pss states, whose buffers free themselves.  Then the
// members go, and with them every DevBuf and PinnedBuf of the context; last
// the base CtxStreams destroys the streams and the events.
ulg_ctx::~ulg_ctx() {
    (void)hipSetDevice(device);
    if (stream) {
        (void)hipStreamSynchronize(stream);
        ulg::graph_reset(this);
    }
    ulg::pss_delete(this);
    ulg::posterior_delete(this);
    ulg::order_mcmc_delete(this);
    delete search;
}

using namespace ulg;

extern "C" {

const char *ulg_version(void) { return "ulg 0.1 (HIP, gfx950/CDNA4)"; }

int ulg_create(const int *device_ids, int ndev, ulg_ctx **out) {
    if (!out) return ULG_ERR_ARG;
    *out = nullptr;
    if (ndev != 1 || !device_ids) return ULG_ERR_ARG;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        fprintf(stderr, "ulg_create: no HIP device available (%s)\n", hipGetErrorString(e));
        return ULG_ERR_HIP;
    }
    if (device_ids[0] < 0 || device_ids[0] >= count) return ULG_ERR_ARG;
    ulg_ctx *c = new ulg_ctx();
    c->device = device_ids[0];
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return ULG_ERR_HIP;
    }
    const auto &b = host_binom();
    if (ensure(c, c->d_binom, b.size()) != ULG_OK ||
        hipMemcpy(c->d_binom.p, b.data(), b.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
        ensure(c, c->d_binom64, host_binom64().size()) != ULG_OK ||
        hipMemcpy(c->d_binom64.p, host_binom64().data(), host_binom64().size() * sizeof(uint64_t),
                  hipMemcpyHostToDevice) != hipSuccess) {
        delete c;
        return ULG_ERR_HIP;
    }
    *out = c;
    return ULG_OK;
}

void ulg_destroy(ulg_ctx *c) {
    if (c) delete c;  // ~ulg_ctx
}

const char *ulg_last_error(const ulg_ctx *c) { return c ? c->err.c_str() : "null context"; }

int ulg_disc_set_ess(ulg_ctx *c, double ess) {
    if (!c) return ULG_ERR_ARG;
    // !(a <= x && x <= b) is also true for a NaN
    if (!(ess >= ulg::kBdeuEssMin && ess <= ulg::kBdeuEssMax))
        return set_err(c, ULG_ERR_ARG, "ulg_disc_set_ess: ess must be finite, 1e-6 <= ess <= 1e6");
    c->disc_ess = ess;
    return ULG_OK;
}

int ulg_set_option(ulg_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return ULG_ERR_ARG;
    std::string msg;
    if (!options_set(c->opt, name, value, &msg)) return set_err(c, ULG_ERR_ARG, msg);
    // the one option with a side effect: a graph captured earlier is dropped
    if (std::strcmp(name, "score_graph") == 0 && !value) graph_reset(c);
    return ULG_OK;
}

int ulg_get_info(ulg_ctx *c, const char *name, int64_t *value) {
    if (!c || !name || !value) return ULG_ERR_ARG;
    // the grid the last ulg_dag_features ran, which the option of that name asks for (0: no launch
    // yet); one of the two option names that do not read back the option
    if (std::strcmp(name, "dagfeat_grid") == 0) {
        *value = c->dagfeat_grid;
        return ULG_OK;
    }
    if (std::strcmp(name, "edges_grid") == 0) {  // ... and the second: the last ulg_order_edges' grid
        *value = c->edges_grid;
        return ULG_OK;
    }
    if (options_get(c->opt, name, value)) return ULG_OK;  // any option, as it stands
    if (std::strcmp(name, "out_of_time") == 0) {
        *value = c->out_of_time;
        return ULG_OK;
    }
    if (std::strcmp(name, "highest_completed_layer") == 0) {
        *value = c->completed_layer;
        return ULG_OK;
    }
    // the last scoring call's device error word: 0 unless a walk over its cap
    // (1), a walk-queue segment overflow (2) or a walk entry past the table (4)
    if (std::strcmp(name, "score_error_word") == 0) {
        *value = (int64_t)c->last_err_word;
        return ULG_OK;
    }
    // scoring calls of this context that captured a launch graph anew (a call
    // whose graph key equals the held one replays it and does not count)
    if (std::strcmp(name, "score_graph_captures") == 0) {
        *value = c->graph_captures;
        return ULG_OK;
    }
    // bytes the process holds through DevBuf / PinnedBuf, every context's together
    if (std::strcmp(name, "device_bytes_live") == 0) {
        *value = g_device_bytes.load();
        return ULG_OK;
    }
    if (std::strcmp(name, "pinned_bytes_live") == 0) {
        *value = g_pinned_bytes.load();
        return ULG_OK;
    }
    // the entries of the unrank tables the context holds
    if (std::strcmp(name, "unrank_lut_entries") == 0) {
        *value = (int64_t)c->lut_cache.total;
        return ULG_OK;
    }
    // the bytes of the launch images the last call built
    if (std::strcmp(name, "lds_image_bytes") == 0) {
        *value = (int64_t)c->plan.image.size();
        return ULG_OK;
    }
    // layer launches of the last ulg_cbic_score that ran the narrow (32-bit) kernels
    if (std::strcmp(name, "narrow_launches") == 0) {
        *value = c->plan.narrow_launches;
        return ULG_OK;
    }
    // the last ulg_disc_score: sets counted in the LDS histogram / in the hash table
    if (std::strcmp(name, "disc_dense_sets") == 0 || std::strcmp(name, "disc_sparse_sets") == 0) {
        *value = c->disc_path_sets[name[5] == 's' ? 1 : 0];
        return ULG_OK;
    }
    // the last ulg_disc_score: sets its prune pass removed (0 with disc_prune off)
    if (std::strcmp(name, "disc_pruned") == 0) {
        *value = c->disc_pruned;
        return ULG_OK;
    }
    // the last ulg_bge_score: sets its prune pass removed (0 with bge_prune off)
    if (std::strcmp(name, "bge_pruned") == 0) {
        *value = c->bge_pruned;
        return ULG_OK;
    }
    // the tables of the last successful ulg_posterior* call (the formula of ulg.h)
    if (std::strcmp(name, "posterior_bytes") == 0) {
        *value = c->posterior_bytes;
        return ULG_OK;
    }
    // batches the last ulg_dag_linear_extensions ran (option "linext_batch")
    if (std::strcmp(name, "linext_batches") == 0) {
        *value = c->linext_batches;
        return ULG_OK;
    }
    // the fNML regret table of the loaded data (0: not built since the last load)
    if (std::strcmp(name, "fnml_table_bytes") == 0) {
        *value = c->fnml_bytes;
        return ULG_OK;
    }
    // the last ulg_disc_mmpc: G^2 tests performed / left out by the reliability rule
    if (std::strcmp(name, "disc_mmpc_tests") == 0 || std::strcmp(name, "disc_mmpc_skipped") == 0) {
        *value = c->disc_mmpc_stat[name[10] == 's' ? 1 : 0];
        return ULG_OK;
    }
    // alternatives held by ulg_cbic_set_constraints
    if (std::strcmp(name, "constraints") == 0) {
        *value = (int64_t)c->cons_var.size();
        return ULG_OK;
    }
    // the last exact A*'s host counters (user space, the calling thread; -1: not granted)
    if (std::strcmp(name, "exact_cycles") == 0) {
        *value = c->exact_pmu[0];
        return ULG_OK;
    }
    if (std::strcmp(name, "exact_instructions") == 0) {
        *value = c->exact_pmu[1];
        return ULG_OK;
    }
    if (std::strcmp(name, "exact_cache_misses") == 0) {
        *value = c->exact_pmu[2];
        return ULG_OK;
    }
    return set_err(c, ULG_ERR_ARG, std::string("unknown info: ") + name);
}

int ulg_stream_wait_event(ulg_ctx *c, void *event) {
    if (!c || !event) return ULG_ERR_ARG;
    ULG_HIP(c, hipSetDevice(c->device));
    ULG_HIP(c, hipStreamWaitEvent(c->stream, (hipEvent_t)event, 0));
    return ULG_OK;
}

int ulg_profile_enable(ulg_ctx *c, int on) {
    if (!c) return ULG_ERR_ARG;
    c->prof = on != 0;
    return ULG_OK;
}

int ulg_profile_select(ulg_ctx *c, const char *names) {
    if (!c) return ULG_ERR_ARG;
    c->prof_only.clear();
    if (names) {
        std::string cur;
        for (const char *p = names;; ++p) {
            if (*p == ',' || *p == 0) {
                if (!cur.empty()) c->prof_only.insert(cur);
                cur.clear();
                if (*p == 0) break;
            } else {
                cur += *p;
            }
        }
    }
    return ULG_OK;
}

int ulg_profile_reset(ulg_ctx *c) {
    if (!c) return ULG_ERR_ARG;
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    c->prof_ms.clear();
    return ULG_OK;
}

int ulg_profile_get(ulg_ctx *c, const char *name, double *avg_ms, int64_t *count, double *total_ms) {
    if (!c || !name) return ULG_ERR_ARG;
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    auto it = c->prof_ms.find(name);
    if (it == c->prof_ms.end() || it->second.empty()) return ULG_ERR_ARG;
    double t = 0;
    for (double v : it->second) t += v;
    if (avg_ms) *avg_ms = t / (double)it->second.size();
    if (count) *count = (int64_t)it->second.size();
    if (total_ms) *total_ms = t;
    return ULG_OK;
}

int ulg_profile_dump(ulg_ctx *c, char *buf, int64_t cap) {
    if (!c || !buf || cap <= 0) return ULG_ERR_ARG;
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    int64_t len = 0;
    buf[0] = 0;
    for (auto &kv : c->prof_ms) {
        double t = 0;
        for (double v : kv.second) t += v;
        int w = snprintf(buf + len, (size_t)(cap - len), "%s %zu %.6f\n", kv.first.c_str(), kv.second.size(), t);
        if (w < 0 || len + w >= cap) break;
        len += w;
    }
    return ULG_OK;
}

}  // extern "C"
