// group.hip — ah_build_forest_group_stream (include/arroy_hip.h, "Device groups"): one forest on every member of a group.
// Trees are independent given the read-only dataset (src/writer.rs:556-591 runs one task per root), so member i builds the
// trees t = i (mod G) with ah_build_forest_stream on its own replica, on a host thread of its own; this file only
// orchestrates: it forwards the members' node batches to the caller's sink under one lock, renumbering them so that the
// caller sees the contract of a single-device streaming build, merges progress, and stops every member on the first error.
// The device work is the existing level-synchronous build of forest.hip.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "common.h"

using namespace ah;

namespace {

constexpr uint32_t kUnassigned = 0xFFFFFFFFu;

struct GroupBuild;

// One member's share: its trees (global index = member + j * G), its renumbering table and its figures.
struct MemberRun {
    GroupBuild *gb = nullptr;
    uint32_t index = 0;
    ah_dataset *ds = nullptr;
    std::vector<uint64_t> seeds;            // tree_seeds of the member's trees, in member-local tree order
    std::vector<uint32_t> roots;            // member-local root ids
    std::vector<uint32_t> global_of;        // member-local node id -> global id (kUnassigned: not seen yet)
    std::vector<ah_stream_node> renumbered; // the batch being forwarded, with global ids
    ah_build_stats stats{};
    int status = AH_OK;
    // progress as last reported by the member (written under GroupBuild::state_mu)
    uint32_t level = 0;
    uint64_t nodes_done = 0, items_routed = 0;
};

struct GroupBuild {
    uint32_t n_members = 0;
    ah_node_batch_fn sink = nullptr;
    void *user = nullptr;
    volatile int stop = 0;                  // every member polls it as its `cancel`
    // the caller's sink and the decision about the call's outcome: one lock, so that no sink call follows the decision
    std::mutex sink_mu;
    bool decided = false;
    int first_status = AH_OK;
    std::string first_error;
    uint32_t next_id = 0;                   // global node ids handed out so far
    // progress and completion, watched by the calling thread
    std::mutex state_mu;
    std::condition_variable cv;
    bool progress_dirty = false;
    uint32_t last_level = 0;
    uint32_t running = 0;

    // the first failure decides the outcome: its status and text are what the call returns; every member stops
    void decide(int status, const char *text) {
        {
            std::lock_guard<std::mutex> lk(sink_mu);
            if (!decided) {
                decided = true;
                first_status = status;
                try {
                    first_error = text ? text : "";
                } catch (...) {
                }
            }
        }
        stop = 1;
    }
};

uint32_t assign(MemberRun &m, uint32_t local, uint32_t global) {
    if (local >= m.global_of.size()) m.global_of.resize(std::max<size_t>((size_t)local + 1, m.global_of.size() * 2), kUnassigned);
    if (m.global_of[local] == kUnassigned) m.global_of[local] = global;
    return m.global_of[local];
}

// The member's sink: renumber the batch into the call's id space and hand it to the caller's sink (same payload: the member's
// pinned buffer, valid during this call).  A root takes the next global id when it first arrives; a split node's children
// take the next two when their parent is forwarded — so ids are dense, unique and children id-consecutive, and a parent
// still precedes its children (the member delivers in that order and one lock serialises all members).
int forward_batch(void *user, const ah_node_batch *batch) {
    MemberRun &m = *static_cast<MemberRun *>(user);
    GroupBuild &gb = *m.gb;
    std::lock_guard<std::mutex> lk(gb.sink_mu);
    if (gb.decided) return 1;
    int rc = 0;
    try {
        const uint32_t G = gb.n_members;
        m.renumbered.resize(batch->n_nodes);
        for (uint64_t i = 0; i < batch->n_nodes; i++) {
            ah_stream_node nd = batch->nodes[i];
            const uint32_t local = nd.id;
            nd.id = assign(m, local, gb.next_id);
            if (nd.id == gb.next_id) gb.next_id++;
            nd.tree = m.index + nd.tree * G;
            if (nd.kind == AH_NODE_SPLIT) {
                const uint32_t l = gb.next_id;
                nd.left = assign(m, nd.left, l);
                nd.right = assign(m, nd.right, l + 1);
                gb.next_id += 2;
            }
            m.renumbered[i] = nd;
        }
        ah_node_batch out = *batch;
        out.nodes = m.renumbered.data();
        rc = gb.sink(gb.user, &out);
    } catch (const std::bad_alloc &) {
        if (!gb.decided) {
            gb.decided = true;
            gb.first_status = AH_ERR_OUT_OF_MEMORY;
            gb.first_error = "ah_build_forest_group_stream: host allocation failed while forwarding a node batch";
        }
        gb.stop = 1;
        return 1;
    }
    if (rc != 0) {
        gb.decided = true;
        gb.first_status = AH_ERR_CANCELLED;
        char buf[96];
        snprintf(buf, sizeof buf, "node sink asked to stop (code %d)", rc);
        try {
            gb.first_error = buf;
        } catch (...) {
        }
        gb.stop = 1;
    }
    return rc;
}

void member_progress(void *user, uint32_t level, uint64_t nodes_done, uint64_t items_routed) {
    MemberRun &m = *static_cast<MemberRun *>(user);
    GroupBuild &gb = *m.gb;
    {
        std::lock_guard<std::mutex> lk(gb.state_mu);
        m.level = level;
        m.nodes_done = std::max(m.nodes_done, nodes_done);
        m.items_routed = std::max(m.items_routed, items_routed);
        gb.last_level = level;
        gb.progress_dirty = true;
    }
    gb.cv.notify_all();
}

void add_stats(ah_build_stats &sum, const ah_build_stats &s) {
    sum.seconds_device += s.seconds_device;
    sum.seconds_margin += s.seconds_margin;
    sum.margin_evaluations += s.margin_evaluations;
    sum.margin_launches += s.margin_launches;
    sum.margin_row_passes += s.margin_row_passes;
    sum.split_nodes += s.split_nodes;
    sum.descendant_nodes += s.descendant_nodes;
    sum.dummy_normals += s.dummy_normals;
    sum.retries += s.retries;
    sum.levels = std::max(sum.levels, s.levels);
    for (int k = 0; k < 8; k++) sum.margin_mode_launches[k] += s.margin_mode_launches[k];
    sum.screened_launches += s.screened_launches;
    sum.screen_fallbacks += s.screen_fallbacks;
    sum.screen_violations += s.screen_violations;
    sum.dense_launches += s.dense_launches;
    sum.dense_columns += s.dense_columns;
    sum.rows_xcd_launches += s.rows_xcd_launches;
    sum.rows_nt_launches += s.rows_nt_launches;
    sum.rows_split_launches += s.rows_split_launches;
    sum.screen8_pairs += s.screen8_pairs;
    sum.screen8_decided += s.screen8_decided;
    sum.screen8b_decided += s.screen8b_decided;
    sum.screen_unavailable += s.screen_unavailable;
    sum.tail_groups += s.tail_groups;
    sum.seconds_setup += s.seconds_setup;
    sum.seconds_after_device += s.seconds_after_device;
    sum.host_blob_recycled += s.host_blob_recycled;
    sum.seconds_reserve += s.seconds_reserve;
    sum.seconds_reserve_wait += s.seconds_reserve_wait;
}

}  // namespace

extern "C" {

int ah_build_forest_group_stream(ah_group *group, const ah_build_options *options, ah_node_batch_fn sink, void *user,
                                 uint32_t *out_roots, ah_build_stats *out_stats, ah_build_stats *out_member_stats) {
    AH_GUARDED("ah_build_forest_group_stream")
    AH_REQUIRE(group, AH_ERR_INVALID_ARGUMENT, "group is NULL");
    AH_REQUIRE(sink, AH_ERR_INVALID_ARGUMENT, "sink is NULL");
    AH_REQUIRE(options && (out_roots || options->n_trees == 0), AH_ERR_INVALID_ARGUMENT, "NULL argument");
    AH_REQUIRE(options->n_trees == 0 || options->tree_seeds, AH_ERR_INVALID_ARGUMENT, "tree_seeds is NULL");
    for (ah_dataset *m : group->members)
        AH_REQUIRE(m->finalized, AH_ERR_NOT_FINALIZED, "group not finalized (call ah_group_finalize)");
    const auto t0 = std::chrono::steady_clock::now();
    DeviceRestore restore_device;  // (every member thread holds its own device; the caller keeps theirs)

    const uint32_t G = (uint32_t)group->members.size();
    const uint32_t n_trees = options->n_trees;
    GroupBuild gb;
    gb.n_members = G;
    gb.sink = sink;
    gb.user = user;
    std::vector<MemberRun> runs(G);
    for (uint32_t i = 0; i < G; i++) {
        MemberRun &m = runs[i];
        m.gb = &gb;
        m.index = i;
        m.ds = group->members[i];
        for (uint32_t t = i; t < n_trees; t += G) m.seeds.push_back(options->tree_seeds[t]);
        m.roots.assign(m.seeds.size(), 0);
    }
    // the host threads of the call's output path are shared between the members
    const long long host_threads = options->max_host_threads ? (long long)options->max_host_threads : tun(TUN_HOST_THREADS);
    const uint32_t per_member_threads = (uint32_t)std::max<long long>(1, host_threads / std::max<uint32_t>(1, std::min(G, n_trees)));

    std::vector<std::thread> threads;
    threads.reserve(G);
    for (uint32_t i = 0; i < G && !gb.stop; i++) {
        MemberRun &m = runs[i];
        if (m.seeds.empty()) continue;
        {
            std::lock_guard<std::mutex> lk(gb.state_mu);
            gb.running++;
        }
        try {
            threads.emplace_back([&m, &gb, options, per_member_threads] {
                ah_build_options opt = *options;
                opt.n_trees = (uint32_t)m.seeds.size();
                opt.tree_seeds = m.seeds.data();
                opt.cancel = &gb.stop;
                opt.progress = options->progress ? member_progress : nullptr;
                opt.progress_user = &m;
                opt.max_host_threads = per_member_threads;
                // (ah_build_forest_stream holds the member's device and turns every failure into a status on this thread)
                m.status = ah_build_forest_stream(m.ds, &opt, forward_batch, &m, m.roots.data(), &m.stats);
                if (m.status != AH_OK) gb.decide(m.status, ah_last_error());
                {
                    std::lock_guard<std::mutex> lk(gb.state_mu);
                    gb.running--;
                }
                gb.cv.notify_all();
            });
        } catch (...) {
            {
                std::lock_guard<std::mutex> lk(gb.state_mu);
                gb.running--;
            }
            gb.decide(AH_ERR_OUT_OF_MEMORY, "ah_build_forest_group_stream: cannot start a host thread for a member");
        }
    }
    // The calling thread watches: it raises the members' stop flag when the caller's cancel flag goes up and reports the
    // members' summed progress (so the caller's progress callback runs on this thread only).
    {
        std::unique_lock<std::mutex> lk(gb.state_mu);
        for (;;) {
            if (options->cancel && *options->cancel && !gb.stop) {
                lk.unlock();
                gb.decide(AH_ERR_CANCELLED, "build cancelled");
                lk.lock();
            }
            if (gb.progress_dirty && options->progress) {
                uint64_t nodes = 0, items = 0;
                for (const MemberRun &m : runs) {
                    nodes += m.nodes_done;
                    items += m.items_routed;
                }
                const uint32_t level = gb.last_level;
                gb.progress_dirty = false;
                lk.unlock();
                options->progress(options->progress_user, level, nodes, items);
                lk.lock();
                continue;
            }
            if (gb.running == 0) break;
            gb.cv.wait_for(lk, std::chrono::milliseconds(1));
        }
    }
    for (std::thread &t : threads) t.join();

    if (gb.decided) {
        set_error("%s", gb.first_error.c_str());
        set_error_status(gb.first_status);
        return gb.first_status;
    }
    // roots in global tree order, in the call's id space
    for (uint32_t i = 0; i < G; i++)
        for (size_t j = 0; j < runs[i].roots.size(); j++) {
            const uint32_t local = runs[i].roots[j];
            AH_REQUIRE(local < runs[i].global_of.size() && runs[i].global_of[local] != kUnassigned, AH_ERR_DEVICE,
                       "member %u never delivered the root of its tree %zu", i, j);
            out_roots[i + j * G] = runs[i].global_of[local];
        }
    if (out_stats) {
        ah_build_stats sum{};
        for (const MemberRun &m : runs) add_stats(sum, m.stats);
        sum.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out_stats = sum;
    }
    if (out_member_stats)
        for (uint32_t i = 0; i < G; i++) out_member_stats[i] = runs[i].stats;
    return AH_OK;
    AH_GUARDED_END
}

}  // extern "C"
