// gymrs_sharded.hip -- the in-process multi-GPU sharder of the C ABI (include/gymrs_amd.h, "one batch over several GPUs").
//
// lanes are fully independent (no cross-lane term anywhere in cartpole.rs:398-483 / mountain_car.rs:398-435), so a batch of
// n_total lanes is cut into contiguous blocks, one engine per block, lane i of block r carrying the global id offset + first[r] + i into the
// Philox counters -- results are identical for any number of blocks.  SURVEY 7.1 step 8: "one host thread + stream per device".  That is what
// this file is: a gymrs_sharded owns k engines and k worker threads; worker r is the ONE thread that ever drives engine r (the reference's
// `&mut self`, core.rs:42-50), bound to that engine's device for its whole life, so k launches are enqueued concurrently and no thread pays
// hipSetDevice or another device's launch cost.  The only exchange of the path, the four statistics doubles, goes through
// gymrs_allreduce_stats_multi (RCCL over xGMI on distinct devices, a host-side sum where shards share a device).
//
// Hand-over of a command: the caller writes the worker's mailbox and bumps its sequence number; a worker that has been idle for less than
// ~100 us is still spinning on that number and starts within a fraction of a microsecond (a per-step loop over a 6 us kernel cannot afford a
// futex wake-up per launch), one that has been idle longer sleeps on a condition variable.  Every call of this file returns when all
// workers have finished ENQUEUEING (gymrs_step* stay asynchronous on each engine's stream); gymrs_sharded_sync waits for the devices.
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>

#include <sched.h>

#include "gymrs_engine_priv.h"

extern "C" gymrs_status gymrs_allreduce_stats_multi(gymrs_engine** shards, int n, double out[4], int* used_rccl);

namespace {

using Job = std::function<gymrs_status(gymrs_engine*&)>;

// one polite spin of a waiting thread (the x86 intrinsic alone made the host code x86-only)
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

// No C++ exception leaves the C ABI or a worker thread (std::vector / std::function / std::thread can throw, and an escaped exception is
// std::terminate for the host process): allocation failures become GYMRS_ENOMEM, anything else GYMRS_EHIP with the exception's text.
template <class F>
gymrs_status guarded(const char* who, F&& f) noexcept
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        try {
            return fail(GYMRS_ENOMEM, std::string(who) + ": host allocation failed");
        } catch (...) {
            return GYMRS_ENOMEM;
        }
    } catch (const std::exception& ex) {
        try {
            return fail(GYMRS_EHIP, std::string(who) + ": " + ex.what());
        } catch (...) {
            return GYMRS_EHIP;
        }
    } catch (...) {
        return GYMRS_EHIP;
    }
}

// "0-3,8,10-11" -> CPU numbers (a sysfs cpulist)
std::vector<int> parse_cpulist(const std::string& text)
{
    std::vector<int> cpus;
    size_t i = 0;
    while (i < text.size()) {
        char* end = nullptr;
        const long lo = std::strtol(text.c_str() + i, &end, 10);
        if (end == text.c_str() + i) break;
        long hi = lo;
        i = (size_t)(end - text.c_str());
        if (i < text.size() && text[i] == '-') {
            hi = std::strtol(text.c_str() + i + 1, &end, 10);
            i = (size_t)(end - text.c_str());
        }
        for (long c = lo; c <= hi && c < 4096; ++c) cpus.push_back((int)c);
        while (i < text.size() && (text[i] == ',' || text[i] == '\n' || text[i] == ' ')) ++i;
    }
    return cpus;
}

// The CPUs local to a HIP device (its PCI function's local_cpulist in sysfs) that this thread may run on; empty when sysfs does not say.
std::vector<int> cpus_near_device(int device, int* numa_node)
{
    *numa_node = -1;
    char bus[64] = {0};
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { // (no runtime call that is KNOWN to fail: its error would sit in the
        (void)hipGetLastError();                                                     //  thread's last-error word until somebody else's launch reads it)
        return {};
    }
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) {
        (void)hipGetLastError();
        return {};
    }
    for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
    auto read = [&](const char* leaf) {
        std::string text;
        const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/" + leaf;
        if (FILE* f = std::fopen(path.c_str(), "r")) {
            char buf[4096];
            const size_t got = std::fread(buf, 1, sizeof(buf) - 1, f);
            buf[got] = 0;
            text = buf;
            std::fclose(f);
        }
        return text;
    };
    const std::string node = read("numa_node");
    if (!node.empty()) *numa_node = std::atoi(node.c_str());
    std::vector<int> local = parse_cpulist(read("local_cpulist"));
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return {};
    std::vector<int> usable;
    for (int c : local)
        if (c >= 0 && c < CPU_SETSIZE && CPU_ISSET(c, &allowed)) usable.push_back(c);
    return usable;
}

struct Worker {
    int index = 0, device = 0;
    uint64_t first = 0, count = 0; // this block's lanes: [first, first + count) of the batch
    gymrs_engine* eng = nullptr;
    std::thread thread;
    // mailbox
    Job job;
    std::atomic<uint64_t> posted{0}, finished{0};
    std::atomic<bool> sleeping{false}, quit{false};
    std::mutex mu;
    std::condition_variable cv;
    gymrs_status status = GYMRS_OK;
    std::string error;
    int pin_slot = 0, pin_sharing = 1; // this worker's place among the workers whose devices share a NUMA node (set before the thread starts)
    int numa_node = -1;                // what the thread found (diagnostics: gymrs_sharded_shard_cpus)
    std::vector<int> pinned;           // the CPUs the thread confined itself to (empty: not pinned)

    // Like gym-rs_amd/sharded.py pin_rank_near_gpu for the process-per-GPU form (VERDICT r5 "next" #4): the ONE thread that drives this block's
    // engine stays on a few CPUs LOCAL to the block's GPU -- a per-step launch costs a thread 2.8 us on its core and 3.1-5.4 us when the scheduler
    // moves it (profiles/r02_cpu_pinning.log), and on a two-socket host a thread on the far socket pays a cross-socket hop per doorbell.  Workers whose
    // GPUs share a node take consecutive blocks of that node's CPUs.  GYMRS_NO_CPU_PIN=1 / GYMRS_NO_NUMA_PIN=1 switch it off; a topology that cannot be
    // read, or too few CPUs, leaves the thread where the caller's mask lets it run.
    void pin_near_device()
    {
        const char* off = std::getenv("GYMRS_NO_CPU_PIN");
        const char* off2 = std::getenv("GYMRS_NO_NUMA_PIN");
        if ((off && off[0] == '1') || (off2 && off2[0] == '1')) return;
        const std::vector<int> usable = cpus_near_device(device, &numa_node);
        if (usable.empty()) return;
        const size_t sharing = (size_t)(pin_sharing < 1 ? 1 : pin_sharing);
        size_t width = usable.size() / sharing;
        if (width > 4) width = 4;
        if (width < 1) return;
        const size_t start = (size_t)pin_slot * width;
        if (start + width > usable.size()) return;
        cpu_set_t mine;
        CPU_ZERO(&mine);
        for (size_t i = 0; i < width; ++i) CPU_SET(usable[start + i], &mine);
        if (sched_setaffinity(0, sizeof(mine), &mine) != 0) return; // (pid 0 = the calling THREAD on Linux)
        pinned.assign(usable.begin() + (long)start, usable.begin() + (long)(start + width));
    }

    void run()
    {
        (void)hipSetDevice(device); // the worker's device for its whole life
        (void)guarded("sharder worker", [&] {
            pin_near_device();
            return GYMRS_OK;
        });
        uint64_t seen = 0;
        for (;;) {
            // a command that follows the last one closely is picked up spinning; otherwise sleep
            bool got = false;
            const auto t0 = std::chrono::steady_clock::now();
            for (uint32_t spin = 0;; ++spin) {
                if (posted.load(std::memory_order_acquire) != seen || quit.load(std::memory_order_acquire)) {
                    got = true;
                    break;
                }
                cpu_relax();
                if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(100)) break;
            }
            if (!got) {
                std::unique_lock<std::mutex> lock(mu);
                sleeping.store(true, std::memory_order_seq_cst);
                cv.wait(lock, [&] { return posted.load(std::memory_order_seq_cst) != seen || quit.load(std::memory_order_seq_cst); });
                sleeping.store(false, std::memory_order_seq_cst);
            }
            if (posted.load(std::memory_order_acquire) == seen) return; // quit with nothing posted
            seen = posted.load(std::memory_order_acquire);
            status = guarded("sharder worker", [&] { return job(eng); });
            if (status != GYMRS_OK) {
                try {
                    error = gymrs_last_error(); // (per thread: carried to the caller's thread by wait())
                } catch (...) {
                    error.clear();
                }
            }
            finished.store(seen, std::memory_order_release);
        }
    }

    void post(Job j)
    {
        job = std::move(j);
        posted.fetch_add(1, std::memory_order_seq_cst);
        if (sleeping.load(std::memory_order_seq_cst)) {
            std::lock_guard<std::mutex> lock(mu);
            cv.notify_one();
        }
    }

    gymrs_status wait()
    {
        const uint64_t want = posted.load(std::memory_order_relaxed);
        for (uint32_t spin = 0; finished.load(std::memory_order_acquire) != want; ++spin) {
            if (spin < 20000u)
                cpu_relax();
            else
                std::this_thread::yield(); // a long call (creation, reset with its copies, a synchronise)
        }
        return status;
    }

    void stop()
    {
        quit.store(true, std::memory_order_seq_cst);
        {
            std::lock_guard<std::mutex> lock(mu);
            cv.notify_one();
        }
        if (thread.joinable()) thread.join();
    }
};

} // namespace

struct gymrs_sharded {
    gymrs_env_kind kind;
    uint64_t n_total = 0, gid0 = 0;
    uint32_t flags = 0;
    std::vector<Worker*> w;
    std::vector<gymrs_engine*> engines;
    int last_used_rccl = -2; // -2: no statistics call yet; 1 RCCL, 0 host-side sum, -1 host-side sum because RCCL was unavailable
    std::string reduce_path;

    // every worker runs its job concurrently; the first failure (lowest shard) is reported on the CALLER's thread
    template <class Make>
    gymrs_status all(Make&& make)
    {
        return guarded("gymrs_sharded", [&]() -> gymrs_status {
            size_t posted = 0;
            gymrs_status st = GYMRS_OK;
            std::string msg;
            try {
                for (; posted < w.size(); ++posted) w[posted]->post(make((int)posted));
            } catch (...) { // (a std::function that could not be allocated: wait for the jobs that WERE posted, then report)
                for (size_t r = 0; r < posted; ++r) (void)w[r]->wait();
                throw;
            }
            for (size_t r = 0; r < w.size(); ++r) {
                const gymrs_status s = w[r]->wait();
                if (s != GYMRS_OK && st == GYMRS_OK) {
                    st = s;
                    msg = "shard " + std::to_string(r) + " (device " + std::to_string(w[r]->device) + "): " + w[r]->error;
                }
            }
            return st == GYMRS_OK ? GYMRS_OK : fail(st, msg);
        });
    }
};

extern "C" {

gymrs_status gymrs_sharded_destroy(gymrs_sharded* h)
{
    if (!h) return GYMRS_OK;
    return guarded("gymrs_sharded_destroy", [&]() -> gymrs_status {
        for (Worker* wk : h->w) { // each engine is destroyed by the thread that drove it, then the thread ends
            wk->post([](gymrs_engine*& e) {
                gymrs_status st = gymrs_engine_destroy(e);
                e = nullptr;
                return st;
            });
            (void)wk->wait();
            wk->stop();
            delete wk;
        }
        delete h;
        return GYMRS_OK;
    });
}

gymrs_status gymrs_sharded_create(gymrs_env_kind kind, uint64_t n_total, uint64_t global_env_offset, int n_shards, const int* devices,
                                  const void* params, uint32_t flags, gymrs_sharded** out)
{
    if (!out) return fail(GYMRS_EINVAL, "gymrs_sharded_create: out is NULL");
    *out = nullptr;
    if (n_shards < 1 || n_shards > 64) return fail(GYMRS_EINVAL, "gymrs_sharded_create: n_shards must be in 1..64");
    if (n_total < (uint64_t)n_shards) return fail(GYMRS_EINVAL, "gymrs_sharded_create: fewer lanes than shards");
    return guarded("gymrs_sharded_create", [&]() -> gymrs_status {
    gymrs_sharded* h = new (std::nothrow) gymrs_sharded();
    if (!h) return fail(GYMRS_ENOMEM, "gymrs_sharded_create: host allocation failed");
    h->kind = kind;
    h->n_total = n_total;
    h->gid0 = global_env_offset;
    h->flags = flags;
    // Contiguous blocks.  The batch's whole 1024-lane tiles are dealt EVENLY (the first `tiles % k` blocks take one more: ADVICE r5 -- rounding every
    // block down and giving the last one the rest made 16376 lanes over 8 blocks 7 x 1024 + 9208), so that every block's arrays start where a tile of
    // the unsharded batch starts; the ragged tail of less than a tile goes to the last block.  A batch of fewer tiles than blocks is cut by lanes.
    // (Nothing depends on the cut -- lanes are independent and carry their GLOBAL id into the Philox counters.)
    const uint64_t tile = 1024, k = (uint64_t)n_shards;
    const uint64_t tiles = n_total / tile, tail = n_total % tile;
    uint64_t first = 0;
    std::vector<int> node_of((size_t)n_shards, -1);
    bool failed = false;
    for (int r = 0; r < n_shards && !failed; ++r) {
        uint64_t count;
        if (tiles >= k)
            count = (tiles / k + ((uint64_t)r < tiles % k ? 1 : 0)) * tile + (r == n_shards - 1 ? tail : 0);
        else
            count = n_total / k + ((uint64_t)r < n_total % k ? 1 : 0);
        Worker* wk = new (std::nothrow) Worker();
        if (!wk) {
            failed = true;
            break;
        }
        wk->index = r;
        wk->device = devices ? devices[r] : r;
        wk->first = first;
        wk->count = count;
        first += count;
        // this worker's place among the workers whose GPUs sit on the same NUMA node (pin_near_device)
        (void)cpus_near_device(wk->device, &node_of[(size_t)r]);
        for (int q = 0; q < r; ++q)
            if (node_of[(size_t)q] == node_of[(size_t)r]) wk->pin_slot += 1;
        h->w.push_back(wk);
    }
    for (Worker* wk : h->w) {
        for (size_t q = 0; q < h->w.size(); ++q)
            if ((int)q != wk->index && node_of[q] == node_of[(size_t)wk->index]) wk->pin_sharing += 1;
    }
    if (!failed) {
        try {
            for (Worker* wk : h->w) wk->thread = std::thread([wk] { wk->run(); });
        } catch (...) { // (std::system_error: no more threads) -- the workers started so far are stopped by destroy
            failed = true;
        }
    }
    if (failed) {
        for (Worker* wk : h->w) {
            wk->stop();
            delete wk;
        }
        h->w.clear();
        delete h;
        return fail(GYMRS_ENOMEM, "gymrs_sharded_create: could not start the worker threads");
    }
    // Engines are created ONE AT A TIME, each by its own worker: creation sets up an HSA queue (where chains are enabled), runs the dispatcher's
    // self-check and times a hand-over, all of which want the device (and, for shards sharing one, the per-device registry) to themselves.
    for (Worker* wk : h->w) {
        const uint64_t off = global_env_offset + wk->first, cnt = wk->count;
        const int dev = wk->device;
        wk->post([=](gymrs_engine*& e) { return gymrs_engine_create(kind, cnt, off, dev, params, flags, &e); });
        if (gymrs_status st = wk->wait()) {
            const std::string msg = "gymrs_sharded_create: shard " + std::to_string(wk->index) + " (device " + std::to_string(dev) + "): " + wk->error;
            gymrs_sharded_destroy(h);
            return fail(st, msg);
        }
    }
    for (Worker* wk : h->w) h->engines.push_back(wk->eng);
    // Like ::new (cartpole.rs:92,120) creation seeds from OS entropy -- ONE seed for the whole batch, or the blocks would not be one batch
    std::random_device rd;
    const uint64_t seed = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    if (gymrs_status st = h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_reset(e, 1, seed, nullptr, nullptr); }; })) {
        const std::string msg = gymrs_last_error();
        gymrs_sharded_destroy(h);
        return fail(st, msg);
    }
    *out = h;
    return GYMRS_OK;
    });
}

gymrs_status gymrs_sharded_count(gymrs_sharded* h, int* n_shards)
{
    if (!h || !n_shards) return fail(GYMRS_EINVAL, "gymrs_sharded_count: NULL argument");
    *n_shards = (int)h->w.size();
    return GYMRS_OK;
}

gymrs_status gymrs_sharded_shard(gymrs_sharded* h, int shard, gymrs_engine** engine, uint64_t* first_lane, uint64_t* n_lanes, int* device)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_shard: handle is NULL");
    if (shard < 0 || shard >= (int)h->w.size()) return fail(GYMRS_EINVAL, "gymrs_sharded_shard: shard index out of range");
    const Worker* wk = h->w[(size_t)shard];
    if (engine) *engine = wk->eng;
    if (first_lane) *first_lane = wk->first;
    if (n_lanes) *n_lanes = wk->count;
    if (device) *device = wk->device;
    return GYMRS_OK;
}

gymrs_status gymrs_sharded_reset(gymrs_sharded* h, int has_seed, uint64_t seed, const float* bounds_low_high, uint64_t* seed_used)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_reset: handle is NULL");
    if (!has_seed) { // seeding.rs:22: a fresh seed from the OS -- drawn once, used by every block
        std::random_device rd;
        seed = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    }
    if (seed_used) *seed_used = seed;
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_reset(e, 1, seed, bounds_low_high, nullptr); }; });
}

gymrs_status gymrs_sharded_step(gymrs_sharded* h, const void* const* actions_dev)
{
    if (!h || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_sharded_step: NULL argument");
    return h->all([=](int r) {
        const void* a = actions_dev[r];
        return [=](gymrs_engine*& e) { return gymrs_step(e, a); };
    });
}

gymrs_status gymrs_sharded_step_many(gymrs_sharded* h, const void* const* actions_dev, uint64_t stride_bytes, uint32_t n_buffers, uint32_t n_steps,
                                     int use_graph)
{
    if (!h || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_sharded_step_many: NULL argument");
    return h->all([=](int r) {
        const void* a = actions_dev[r];
        return [=](gymrs_engine*& e) { return gymrs_step_many(e, a, stride_bytes, n_buffers, n_steps, use_graph); };
    });
}

gymrs_status gymrs_sharded_fill_actions(gymrs_sharded* h, void* const* actions_dev, uint64_t seed, uint64_t t)
{
    if (!h || !actions_dev) return fail(GYMRS_EINVAL, "gymrs_sharded_fill_actions: NULL argument");
    return h->all([=](int r) {
        void* a = actions_dev[r];
        return [=](gymrs_engine*& e) { return gymrs_fill_actions(e, a, seed, t); };
    });
}

// The fused random-policy rollout (gymrs_rollout) on every block: the action stream is keyed by GLOBAL lane ids, so the batch does what one engine would.
gymrs_status gymrs_sharded_rollout(gymrs_sharded* h, uint32_t n_steps, uint64_t action_seed, uint64_t action_t0)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_rollout: handle is NULL");
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_rollout(e, n_steps, action_seed, action_t0); }; });
}

// The closed-loop calls on every block: the same policy set everywhere, keyed by GLOBAL lane ids like the action stream above.
gymrs_status gymrs_sharded_set_policy(gymrs_sharded* h, const gymrs_policy_desc* d, const float* weights_host)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_set_policy: handle is NULL");
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_set_policy(e, d, weights_host); }; });
}

// The same exploration settings on every block: the draw is keyed by GLOBAL lane ids and the blocks' ticks move together.
gymrs_status gymrs_sharded_set_exploration(gymrs_sharded* h, const gymrs_exploration* x)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_set_exploration: handle is NULL");
    const bool remove = x == nullptr;
    const gymrs_exploration settings = remove ? gymrs_exploration{0, 0, 0} : *x; // by value into the workers
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_set_exploration(e, remove ? nullptr : &settings); }; });
}

// ... and the same sampling settings.
gymrs_status gymrs_sharded_set_sampling(gymrs_sharded* h, const gymrs_sampling* x)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_set_sampling: handle is NULL");
    const bool remove = x == nullptr;
    const gymrs_sampling settings = remove ? gymrs_sampling{0, 0.0f, 0} : *x; // by value into the workers
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_set_sampling(e, remove ? nullptr : &settings); }; });
}

gymrs_status gymrs_sharded_rollout_policy(gymrs_sharded* h, uint32_t n_steps)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_rollout_policy: handle is NULL");
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_rollout_policy(e, n_steps); }; });
}

gymrs_status gymrs_sharded_rollout_policy_fitness(gymrs_sharded* h, uint32_t n_steps)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_rollout_policy_fitness: handle is NULL");
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_rollout_policy_fitness(e, n_steps); }; });
}

gymrs_status gymrs_sharded_policy_fitness_clear(gymrs_sharded* h)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_policy_fitness_clear: handle is NULL");
    return h->all([](int) { return [](gymrs_engine*& e) { return gymrs_policy_fitness_clear(e); }; });
}

// Records [first, first + count) of the batch: every block's records (read by its worker), added up on the caller's thread.
gymrs_status gymrs_sharded_get_policy_fitness(gymrs_sharded* h, uint32_t first, uint32_t count, gymrs_policy_fitness* host_out)
{
    if (!h || !host_out) return fail(GYMRS_EINVAL, "gymrs_sharded_get_policy_fitness: NULL argument");
    return guarded("gymrs_sharded_get_policy_fitness", [&]() -> gymrs_status {
        const size_t k = h->w.size();
        // (count == 0 is a range check and a synchronise on every block, as on one engine: one spare record per block keeps the pointers non-NULL)
        std::vector<gymrs_policy_fitness> part(k * (size_t)count + k);
        gymrs_policy_fitness* parts = part.data();
        if (gymrs_status st = h->all([=](int r) {
                gymrs_policy_fitness* mine = parts + (size_t)r * count;
                return [=](gymrs_engine*& e) { return gymrs_get_policy_fitness(e, first, count, mine); };
            }))
            return st;
        for (uint32_t p = 0; p < count; ++p) {
            gymrs_policy_fitness sum = {0, 0, 0, 0};
            for (size_t r = 0; r < k; ++r) {
                const gymrs_policy_fitness& f = parts[r * count + p];
                sum.reward_sum += f.reward_sum;
                sum.episodes += f.episodes;
                sum.done += f.done;
                sum.truncated += f.truncated;
            }
            host_out[p] = sum;
        }
        return GYMRS_OK;
    });
}

// gymrs_rollout_closed_loop on every block (the flags pass through: GYMRS_CLOSED_LOOP_LANE_PARAMS steps every block's lanes with the block's table and
// index).  A trajectory is an array of ONE engine's lanes: ask the blocks themselves for it.
gymrs_status gymrs_sharded_rollout_closed_loop(gymrs_sharded* h, const gymrs_closed_loop_desc* d)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_rollout_closed_loop: handle is NULL");
    if (!d) return fail(GYMRS_EINVAL, "gymrs_sharded_rollout_closed_loop: NULL desc");
    if (d->record) return fail(GYMRS_EINVAL, "gymrs_sharded_rollout_closed_loop: record must be NULL (the blocks live on several devices)");
    const gymrs_closed_loop_desc desc = *d; // by value into the workers
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_rollout_closed_loop(e, &desc); }; });
}

// Episodic evaluation on every block (the flags pass through: GYMRS_EVAL_LANE_PARAMS plays every block's table).  The per-episode lengths are an array of ONE engine's lanes: ask the blocks themselves for them.
gymrs_status gymrs_sharded_evaluate_policy(gymrs_sharded* h, const gymrs_eval_desc* d)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_evaluate_policy: handle is NULL");
    if (!d) return fail(GYMRS_EINVAL, "gymrs_sharded_evaluate_policy: NULL desc");
    if (d->lengths_dev) return fail(GYMRS_EINVAL, "gymrs_sharded_evaluate_policy: lengths_dev must be NULL (the blocks live on several devices)");
    const gymrs_eval_desc desc = *d;
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_evaluate_policy(e, &desc); }; });
}

// Records [first, first + count) of the batch: every block's records (read by its worker), merged on the caller's thread: sums added,
// the min of the mins, the max of the maxes (a block without a lane of the policy holds the identity).
gymrs_status gymrs_sharded_get_policy_eval(gymrs_sharded* h, uint32_t first, uint32_t count, gymrs_policy_eval* host_out)
{
    if (!h || !host_out) return fail(GYMRS_EINVAL, "gymrs_sharded_get_policy_eval: NULL argument");
    return guarded("gymrs_sharded_get_policy_eval", [&]() -> gymrs_status {
        const size_t k = h->w.size();
        std::vector<gymrs_policy_eval> part(k * (size_t)count + k); // (one spare record per block keeps the pointers non-NULL at count == 0)
        gymrs_policy_eval* parts = part.data();
        if (gymrs_status st = h->all([=](int r) {
                gymrs_policy_eval* mine = parts + (size_t)r * count;
                return [=](gymrs_engine*& e) { return gymrs_get_policy_eval(e, first, count, mine); };
            }))
            return st;
        for (uint32_t p = 0; p < count; ++p) {
            gymrs_policy_eval m = {0, 0, 0, 0, 0, 0, INT64_MAX, INT64_MIN};
            for (size_t r = 0; r < k; ++r) {
                const gymrs_policy_eval& f = parts[r * count + p];
                m.return_sum = (int64_t)((uint64_t)m.return_sum + (uint64_t)f.return_sum);
                m.return_sq_sum += f.return_sq_sum;
                m.episodes += f.episodes;
                m.done += f.done;
                m.truncated += f.truncated;
                m.steps += f.steps;
                m.return_min = f.return_min < m.return_min ? f.return_min : m.return_min;
                m.return_max = f.return_max > m.return_max ? f.return_max : m.return_max;
            }
            host_out[p] = m;
        }
        return GYMRS_OK;
    });
}

// `env.gravity = ...` for every lane of the batch (gymrs_set_params on every block).
gymrs_status gymrs_sharded_set_params(gymrs_sharded* h, const void* params)
{
    if (!h || !params) return fail(GYMRS_EINVAL, "gymrs_sharded_set_params: NULL argument");
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_set_params(e, params); }; });
}

// Per-lane physics on a batch: the same rows on every block, the index in BATCH lane numbering (cut like gymrs_sharded_get_state's ranges).
gymrs_status gymrs_sharded_set_param_table(gymrs_sharded* h, const void* rows, uint32_t k)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_set_param_table: handle is NULL");
    return h->all([=](int) { return [=](gymrs_engine*& e) { return gymrs_set_param_table(e, rows, k); }; });
}

gymrs_status gymrs_sharded_get_param_table(gymrs_sharded* h, void* rows_out, uint32_t capacity, uint32_t* k)
{
    if (!h || !k) return fail(GYMRS_EINVAL, "gymrs_sharded_get_param_table: NULL argument");
    return h->all([=](int r) {
        return [=](gymrs_engine*& e) -> gymrs_status { return r == 0 ? gymrs_get_param_table(e, rows_out, capacity, k) : GYMRS_OK; };
    });
}

gymrs_status gymrs_sharded_set_param_index(gymrs_sharded* h, uint64_t first, uint64_t count, const uint16_t* index_host)
{
    if (!h || !index_host) return fail(GYMRS_EINVAL, "gymrs_sharded_set_param_index: NULL argument");
    if (first > h->n_total || count > h->n_total - first) return fail(GYMRS_EINVAL, "gymrs_sharded_set_param_index: lane range out of bounds");
    return h->all([=](int r) {
        const Worker* wk = h->w[(size_t)r];
        const uint64_t lo = first > wk->first ? first : wk->first;
        const uint64_t hi = (first + count) < (wk->first + wk->count) ? (first + count) : (wk->first + wk->count);
        return [=](gymrs_engine*& e) -> gymrs_status { // (a block the range misses still says whether it has a table)
            return lo >= hi ? gymrs_set_param_index(e, 0, 0, index_host) : gymrs_set_param_index(e, lo - wk->first, hi - lo, index_host + (lo - first));
        };
    });
}

gymrs_status gymrs_sharded_get_param_index(gymrs_sharded* h, uint64_t first, uint64_t count, uint16_t* index_out)
{
    if (!h || !index_out) return fail(GYMRS_EINVAL, "gymrs_sharded_get_param_index: NULL argument");
    if (first > h->n_total || count > h->n_total - first) return fail(GYMRS_EINVAL, "gymrs_sharded_get_param_index: lane range out of bounds");
    return h->all([=](int r) {
        const Worker* wk = h->w[(size_t)r];
        const uint64_t lo = first > wk->first ? first : wk->first;
        const uint64_t hi = (first + count) < (wk->first + wk->count) ? (first + count) : (wk->first + wk->count);
        return [=](gymrs_engine*& e) -> gymrs_status {
            return lo >= hi ? gymrs_get_param_index(e, 0, 0, index_out) : gymrs_get_param_index(e, lo - wk->first, hi - lo, index_out + (lo - first));
        };
    });
}

gymrs_status gymrs_sharded_sync(gymrs_sharded* h)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_sync: handle is NULL");
    return h->all([](int) { return [](gymrs_engine*& e) { return gymrs_sync(e); }; });
}

gymrs_status gymrs_sharded_stats_clear(gymrs_sharded* h)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_stats_clear: handle is NULL");
    return h->all([](int) { return [](gymrs_engine*& e) { return gymrs_stats_clear(e); }; });
}

gymrs_status gymrs_sharded_stats(gymrs_sharded* h, double out[4])
{
    if (!h || !out) return fail(GYMRS_EINVAL, "gymrs_sharded_stats: NULL argument");
    // The workers are idle (every call of this file returns after its jobs): the calling thread may drive all engines for this one call --
    // RCCL's grouped form wants ONE thread to issue every rank's all-reduce.
    int used = 0;
    if (gymrs_status st = gymrs_allreduce_stats_multi(h->engines.data(), (int)h->engines.size(), out, &used)) return st;
    h->last_used_rccl = used;
    h->reduce_path = used > 0 ? "rccl" : (used == 0 ? "host" : std::string("host (") + gymrs_last_error() + ")");
    return GYMRS_OK;
}

gymrs_status gymrs_sharded_get_state(gymrs_sharded* h, uint64_t first, uint64_t count, float* host_out)
{
    if (!h || !host_out) return fail(GYMRS_EINVAL, "gymrs_sharded_get_state: NULL argument");
    if (first > h->n_total || count > h->n_total - first) return fail(GYMRS_EINVAL, "gymrs_sharded_get_state: lane range out of bounds");
    // SoA over the REQUESTED lanes: dim arrays of `count` floats back to back, like gymrs_get_state
    const int dim = h->kind == GYMRS_CARTPOLE ? 4 : 2;
    return h->all([=](int r) {
        const Worker* wk = h->w[(size_t)r];
        const uint64_t lo = first > wk->first ? first : wk->first;
        const uint64_t hi = (first + count) < (wk->first + wk->count) ? (first + count) : (wk->first + wk->count);
        return [=](gymrs_engine*& e) -> gymrs_status {
            if (lo >= hi) return GYMRS_OK;
            std::vector<float> tmp((size_t)(hi - lo) * (size_t)dim);
            if (gymrs_status st = gymrs_get_state(e, lo - wk->first, hi - lo, tmp.data())) return st;
            for (int j = 0; j < dim; ++j)
                std::memcpy(host_out + (size_t)j * count + (lo - first), tmp.data() + (size_t)j * (hi - lo), (size_t)(hi - lo) * sizeof(float));
            return GYMRS_OK;
        };
    });
}

gymrs_status gymrs_sharded_get_step_result(gymrs_sharded* h, uint64_t first, uint64_t count, float* reward, uint8_t* done, uint8_t* truncated)
{
    if (!h) return fail(GYMRS_EINVAL, "gymrs_sharded_get_step_result: handle is NULL");
    if (first > h->n_total || count > h->n_total - first) return fail(GYMRS_EINVAL, "gymrs_sharded_get_step_result: lane range out of bounds");
    return h->all([=](int r) {
        const Worker* wk = h->w[(size_t)r];
        const uint64_t lo = first > wk->first ? first : wk->first;
        const uint64_t hi = (first + count) < (wk->first + wk->count) ? (first + count) : (wk->first + wk->count);
        return [=](gymrs_engine*& e) -> gymrs_status {
            if (lo >= hi) return GYMRS_OK;
            const uint64_t o = lo - first;
            return gymrs_get_step_result(e, lo - wk->first, hi - lo, reward ? reward + o : nullptr, done ? done + o : nullptr,
                                         truncated ? truncated + o : nullptr);
        };
    });
}

// How the last gymrs_sharded_stats summed: "rccl" (grouped all-reduce over the shards' communicators), "host" (shards share a device, or one
// shard), or "none" before the first call.
const char* gymrs_sharded_reduce_path(gymrs_sharded* h)
{
    if (!h || h->last_used_rccl == -2) return "none";
    return h->reduce_path.c_str();
}

} // extern "C"
