// The plan-time races and the plan cache (TAMD_PLAN_CACHE=<file>) that remembers what they decided, shared by the planners
// (graph_plan_conv.hip, graph_plan_pairs.hip, graph_u8.hip, graph_f32.hip).  Split out of graph.hip in round 6.
#include "graph.h"
#include "graph_internal.h"
#include "env.h"

#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <mutex>

#include "epilogue.h"

namespace tamd {

// ---- plan cache (TAMD_PLAN_CACHE=<file>): what the plan-time autotune decided, "<site>|<node>|<shape>" -> choice ---------------
// A first prerun measures as usual and writes the file; later preruns of the same model take the recorded choices WITHOUT
// launching anything -- a profiler then sees the run's own launches only (round 2's rocprofv3 CSVs were 99 % autotune
// dispatches), the plan no longer depends on one box's timing noise, and prerun drops from seconds to the packing time.
// The table is process-wide (graphs of one process share it) and guarded by a mutex; a file that changed on disk since it was
// read (size or modification time) is read again at the next lookup.
struct PlanCache {
    bool loaded = false, dirty = false;
    std::string path;
    long long stamp = 0;                                  // size ^ mtime of the file as read / written
    std::map<std::string, std::string> kv;     // the file's entries + this process's
    std::map<std::string, std::string> mine;   // what THIS process decided since the file was read (merged over the file at flush)
};
static std::mutex g_plan_cache_mu;
static long long file_stamp(const std::string& path)
{
    struct stat st;
    if (path.empty() || stat(path.c_str(), &st) != 0) return 0;
    return (long long)st.st_size * 1000003ll ^ (long long)st.st_mtim.tv_sec * 1000000007ll ^ (long long)st.st_mtim.tv_nsec;
}
// first line of a plan file: what the choices were made FOR.  A file written by another library version, for another
// architecture or with another candidate list is ignored as a whole (and overwritten at the next flush): a stale choice
// could name a configuration this build no longer launches
static std::string plan_cache_header()
{
    return std::string("#tamd-plan v2 gfx950 ") + tamd_version() + " gemm" + std::to_string(conv_igemm_num_cfgs()) + "/" + std::to_string(conv_pgemm_num_variants())
           + " u8" + std::to_string(conv_u8_gemm_num_cfgs()) + "/" + std::to_string(conv_u8_patch_num_cfgs());
}
static void plan_cache_read(const std::string& path, std::map<std::string, std::string>* kv)
{
    FILE* f = path.empty() ? nullptr : fopen(path.c_str(), "r");
    if (!f) return;
    char line[512];
    bool first = true, ok = false;
    while (fgets(line, sizeof(line), f)) {
        std::string l = line;
        while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
        if (first) { first = false; ok = l == plan_cache_header(); if (!ok) break; continue; }
        const size_t tab = l.find('\t');
        if (tab == std::string::npos) continue;
        (*kv)[l.substr(0, tab)] = l.substr(tab + 1);
    }
    fclose(f);
    if (!ok) kv->clear();
}
static PlanCache& plan_cache_locked()                     // call with g_plan_cache_mu held
{
    static PlanCache pc;
    const char* p = getenv("TAMD_PLAN_CACHE");
    const std::string want = p ? p : "";
    if (!pc.loaded || pc.path != want || (!pc.dirty && file_stamp(want) != pc.stamp)) {
        pc = PlanCache();
        pc.loaded = true; pc.path = want; pc.stamp = file_stamp(want);
        plan_cache_read(want, &pc.kv);
    }
    return pc;
}
static bool plan_cache_get(const std::string& key, std::string* v)
{
    std::lock_guard<std::mutex> lk(g_plan_cache_mu);
    PlanCache& pc = plan_cache_locked();
    auto it = pc.kv.find(key);
    if (pc.path.empty() || it == pc.kv.end()) return false;
    *v = it->second;
    return true;
}
static void plan_cache_put(const std::string& key, const std::string& v)
{
    std::lock_guard<std::mutex> lk(g_plan_cache_mu);
    PlanCache& pc = plan_cache_locked();
    if (pc.path.empty()) return;
    pc.kv[key] = v;
    pc.mine[key] = v;
    pc.dirty = true;
}
// Several processes may share one file (the ranks of a multi-GPU job): the entries on disk are merged with this process's own
// decisions (ours win), written to a temporary file and renamed over the old one -- a reader sees the old file or the new one,
// never half of either.
void plan_cache_flush()
{
    std::lock_guard<std::mutex> lk(g_plan_cache_mu);
    PlanCache& pc = plan_cache_locked();
    if (pc.path.empty() || !pc.dirty) return;
    std::map<std::string, std::string> merged;
    plan_cache_read(pc.path, &merged);
    for (auto& e : pc.mine) merged[e.first] = e.second;
    const std::string tmp = pc.path + ".tmp." + std::to_string((long)getpid());
    if (FILE* f = fopen(tmp.c_str(), "w")) {
        fprintf(f, "%s\n", plan_cache_header().c_str());
        for (auto& e : merged) fprintf(f, "%s\t%s\n", e.first.c_str(), e.second.c_str());
        fclose(f);
        if (rename(tmp.c_str(), pc.path.c_str()) != 0) (void)remove(tmp.c_str());
    }
    pc.kv = merged;
    pc.dirty = false;
    pc.stamp = file_stamp(pc.path);
}

// ---- plan-time races: time the candidates, keep the incumbent unless another one wins by the margin, remember the winner -------
// plan-time autotune: candidates of a graph whose pass moves far more bytes than the L2s hold are timed COLD -- every timed
// launch behind a fill of kL2FlushBytes (l2_flush_buffer(): one per device, kept for the life of the process) -- because that
// is how they run inside a pass; small graphs (batch-1 classifiers live in the L2s from step to step) keep back-to-back timing
constexpr size_t kL2FlushBytes = 64u << 20;

static void* l2_flush_buffer()
{
    static std::mutex mu;
    static std::map<int, void*> per_dev;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto it = per_dev.find(dev);
    if (it != per_dev.end()) return it->second;
    void* p = nullptr;
    if (hipMalloc(&p, kL2FlushBytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
    per_dev[dev] = p;
    return p;
}

static bool autotune_cold(tamd_graph* g)
{
    if (g->autotune_cold < 0) {
        const char* e = exp_env("TAMD_AUTOTUNE_COLD");              // 0: always warm, 1: always cold
        size_t bytes = 0;
        for (const HTensor& t : g->tensors)
            bytes += (t.ttype == TAMD_TT_VAR || t.ttype == TAMD_TT_INPUT) && t.n > 0 ? (size_t)t.n * t.h * t.w * (t.cs > 0 ? t.cs : t.c) : t.elems() * (t.dtype == TAMD_DT_FP32 ? 4 : 1);
        g->autotune_cold = e ? (atoi(e) != 0) : bytes > (size_t)(48u << 20);      // tensors + weights of one pass vs 32 MB of L2
    }
    return g->autotune_cold == 1;
}

// one candidate the way it runs inside a pass: the fill evicts its weights (and everything else) from the L2s, the step planned
// just before it -- as a rule the producer of its input -- runs again and leaves that input where a pass leaves it, then the
// candidate is timed on its own.  Five samples, the slowest dropped.
static int time_cold(tamd_graph* g, void* flush, const std::function<hipError_t()>& launch, float* ms_out)
{
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    const Step* prev = nullptr;
    for (size_t i = g->steps.size(); i-- > 0 && !prev;)
        if (!g->steps[i].once) prev = &g->steps[i];
    float tot = 0.f, worst = 0.f;
    const int reps = 5;
    for (int it = 0; it < reps; it++) {
        float t = 0;
        HIPCHK(hipMemsetAsync(flush, it, kL2FlushBytes, g->stream));
        if (prev) (void)prev->fn(g->stream);
        HIPCHK(hipEventRecord(e0, g->stream));
        (void)launch();
        HIPCHK(hipEventRecord(e1, g->stream));
        HIPCHK(hipEventSynchronize(e1));
        HIPCHK(hipEventElapsedTime(&t, e0, e1));
        tot += t;
        worst = std::max(worst, t);
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    (void)hipGetLastError();
    *ms_out = (tot - worst) / (reps - 1);
    return 0;
}

// average duration of one launch of `fn` on the graph's stream (plan-time autotune): back to back, or each launch behind an
// L2-evicting fill (autotune_cold)
static int time_fn(tamd_graph* g, const std::function<hipError_t(hipStream_t)>& fn, float* ms_out)
{
    hipEvent_t e0, e1;
    *ms_out = 1e30f;
    hipError_t err = fn(g->stream);
    if (err == hipSuccess) err = fn(g->stream);
    if (err != hipSuccess) { (void)hipGetLastError(); return 0; }
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    if (void* flush = autotune_cold(g) ? l2_flush_buffer() : nullptr) {
        hipEventDestroy(e0); hipEventDestroy(e1);
        return time_cold(g, flush, [&]() { return fn(g->stream); }, ms_out);
    }
    // best of two timed bursts (the ranking decides the plan: run-to-run noise of a single burst showed up as 5-10 % swings of
    // whole-model times); short kernels (batch-1 layers are a few microseconds) get longer bursts
    float ms = 1e30f;
    int reps = 8;
    for (int round = 0; round < 3; round++) {
        float t = 0;
        HIPCHK(hipEventRecord(e0, g->stream));
        for (int it = 0; it < reps; it++) (void)fn(g->stream);
        HIPCHK(hipEventRecord(e1, g->stream));
        HIPCHK(hipEventSynchronize(e1));
        HIPCHK(hipEventElapsedTime(&t, e0, e1));
        t /= reps;
        if (round == 0 && t <= 0.02f) { reps = 40; continue; }      // re-measure short kernels with a longer burst
        ms = std::min(ms, t);
        if (round == 0) round = 1;                                  // long kernel: bursts 0 and 2
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    *ms_out = ms;
    return 0;
}

bool autotune_enabled()
{
    const char* at_env = getenv("TAMD_AUTOTUNE");
    return !(at_env && atoi(at_env) == 0);
}

int plan_cached(const std::string& key, const std::vector<RaceCand>& cands)
{
    std::string v;
    if (key.empty() || !plan_cache_get(key, &v)) return -1;
    for (size_t c = 0; c < cands.size(); c++)
        if (cands[c].tag == v) return !cands[c].live || cands[c].live() ? (int)c : -1;
    return -1;
}

int plan_race(tamd_graph* g, const std::string& node, const std::vector<RaceCand>& cands, const std::string& key, float margin, bool tune)
{
    if (!tune) return 0;
    const int hit = plan_cached(key, cands);
    if (hit >= 0) return hit;
    // a few timed launches of each candidate on the real buffers (outputs are overwritten again by the first real run)
    int best = 0;
    float best_ms = 1e30f;
    for (size_t c = 0; c < cands.size(); c++) {
        float ms;
        if (time_fn(g, cands[c].fn, &ms)) return -1;
        if (getenv("TAMD_DEBUG"))
            fprintf(stderr, ms > 1e29f ? "[tamd] %s: %s does not launch\n" : "[tamd] %s: %s %.2f us\n", node.c_str(),
                    (cands[c].name.empty() ? cands[c].tag : cands[c].name).c_str(), 1e3 * ms);
        if (ms > 1e29f) continue;
        if (best_ms > 1e29f || ms < best_ms * margin) { best_ms = ms; best = (int)c; }
    }
    if (!key.empty()) plan_cache_put(key, cands[best].tag);
    return best;
}

}  // namespace tamd
