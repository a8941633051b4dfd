// mapcaller_amd/csrc/mcx_shards.h — a run spread over several shards: the exchange between the host threads of one process, the rounds' protocol
// (Shards), and what the formatter and the thread that talks to the other shards tell each other (Places).
#pragma once
#include <map>
#include "mcx_pool.h"
#include "mcx_internal.h"

namespace mcx { namespace files {

// ---- exchange between the host threads of one process (mapcaller-mi355x -gpus N) ------------------------
struct Rendezvous {
    std::mutex m; std::condition_variable cv;
    int size = 0, arrived = 0, left = 0;
    uint64_t gen = 0, gen_out = 0;
    std::vector<const void *> ptr;
};
struct LocalPeer { Rendezvous *rv; int rank; };

inline int local_allgather(void *user, const void *send, void *recv, uint64_t bytes)
{
    LocalPeer *p = (LocalPeer *)user;
    Rendezvous &rv = *p->rv;
    {
        std::unique_lock<std::mutex> l(rv.m);
        rv.ptr[(size_t)p->rank] = send;
        const uint64_t g = rv.gen;
        if (++rv.arrived == rv.size) { rv.arrived = 0; rv.gen++; rv.cv.notify_all(); }
        else rv.cv.wait(l, [&] { return rv.gen != g; });
    }
    for (int r = 0; r < rv.size; r++) memcpy((uint8_t *)recv + (size_t)r * bytes, rv.ptr[(size_t)r], bytes);
    { // nobody's send buffer may change before everyone has copied it
        std::unique_lock<std::mutex> l(rv.m);
        const uint64_t g = rv.gen_out;
        if (++rv.left == rv.size) { rv.left = 0; rv.gen_out++; rv.cv.notify_all(); }
        else rv.cv.wait(l, [&] { return rv.gen_out != g; });
    }
    return 0;
}

// ---- one round of a run spread over several shards ------------------------------------------------------
// Round j holds batches j*N .. j*N+N-1, one per shard.  The shards exchange (a) what each has in the round,
// (b) per-chunk pair sums until the ONE insert-size trajectory of the input stream (ReadMapping.cpp:462,
// :538-539) has been walked over all of them and no shard had to re-run a pair, (c) with -vcf, the duplicate-check
// keys, so that the cap admits reads in input order across shards (AlignmentProfile.cpp:76-77), (d) the bytes of
// SAM text their batches of an earlier round came to, so that every shard writes at its final place.  Every shard
// makes the same sequence of exchange calls whatever it holds; a failing shard keeps taking part until the
// round's next message has told the others.
struct Shards {
    const mcx_exchange *x;
    uint32_t slot_stride;   // reads a batch holds at most
    uint32_t cap_chunks;
    std::vector<uint8_t> recv;
    std::vector<uint32_t> msg;
    std::vector<uint64_t> all_keys, pad_keys;
    struct Head { int32_t rc; uint32_t n_pair, n_single, last; };

    int gather(const void *send, size_t bytes)
    {
        recv.resize(bytes * (size_t)x->size);
        return x->allgather(x->user, send, recv.data(), bytes) ? mcx_set_error(MCX_ERR_DEVICE, "the exchange between the shards failed") : 0;
    }
    // any shard's failure ends the run on all of them
    int agree(int my_rc)
    {
        int32_t v = my_rc;
        if (int e = gather(&v, sizeof v)) return e;
        if (my_rc) return my_rc;
        for (int r = 0; r < x->size; r++) { int32_t o; memcpy(&o, recv.data() + (size_t)r * sizeof o, sizeof o); if (o) return mcx_set_error(o, "shard " + std::to_string(r) + " failed"); }
        return 0;
    }

    // closes a part of the round: -vcf bookkeeping with the keys of every shard, or the plain end
    int finish_part(mcx_ctx *c, bool mine, bool profile, mcx_stats *stats, int rc)
    {
        if (!profile) { if (rc == 0 && mine) rc = mcx_batch_end(c, stats); return agree(rc); }
        const uint64_t *keys = nullptr; uint64_t nk = 0;
        if (rc == 0 && mine) rc = mcx_batch_end_keys(c, stats, &keys, &nk);
        if (rc) nk = 0;
        struct { int32_t rc; uint32_t pad; uint64_t n; } h = {rc, 0, nk}, o;
        if (int e = gather(&h, sizeof h)) return e;
        uint64_t most = 0, total = 0;
        std::vector<uint64_t> cnt((size_t)x->size);
        int bad = rc;
        for (int r = 0; r < x->size; r++) { memcpy(&o, recv.data() + (size_t)r * sizeof o, sizeof o); cnt[(size_t)r] = o.n; most = std::max(most, o.n); total += o.n; if (!bad && o.rc) bad = mcx_set_error(o.rc, "shard " + std::to_string(r) + " failed"); }
        if (bad) return bad;
        if (most == 0) { if (mine) rc = mcx_batch_accumulate(c, nullptr, 0, slot_stride, (uint32_t)x->rank); return agree(rc); }
        pad_keys.assign((size_t)most, ~0ull);
        for (uint64_t i = 0; i < nk; i++) pad_keys[(size_t)i] = keys[i] + (uint64_t)x->rank * slot_stride; // the read's number within the round
        if (int e = gather(pad_keys.data(), (size_t)most * sizeof(uint64_t))) return e;
        all_keys.clear(); all_keys.reserve((size_t)total);
        for (int r = 0; r < x->size; r++) {
            const uint64_t *p = (const uint64_t *)(recv.data() + (size_t)r * (size_t)most * sizeof(uint64_t));
            all_keys.insert(all_keys.end(), p, p + cnt[(size_t)r]);
        }
        rc = mcx_batch_accumulate(c, all_keys.data(), all_keys.size(), slot_stride, mine ? (uint32_t)x->rank : 0xFFFFFFFFu);
        return agree(rc);
    }

    // The paired part of a round.  n = this shard's reads (0: none), in HBM already; avg = the run's state {avgDist, pairs, distance, reads}.
    int pairs(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n, int64_t read_base, int64_t avg[4], bool profile,
              mcx_aln *d_aln, uint32_t *d_cig, mcx_stats *stats)
    {
        int rc = 0;
        if (n) rc = mcx_batch_begin(c, d_bases, d_off, n, 1, (int32_t)((uint32_t)avg[0] * 1.5), read_base, d_aln, d_cig, stats);
        // What the shards tell each other per exchange: {status, chunks, pairs re-run, -, proper pairs, their summed distance} — totals, not the
        // chunks' sums: a shard walks its own chunks from the round's state plus the totals of the shards before it in input order (below).
        struct Msg { uint32_t rc, n_chunks, n_redo, pad; int64_t pairs, dist; } mine, o;
        uint32_t n_redo = 0xFFFFFFFFu; // "not replayed yet"
        int64_t st[3] = {avg[0], avg[1], avg[2]};
        std::vector<int32_t> est;
        for (int iter = 0;; iter++) {
            uint32_t nc = 0;
            int64_t tot[2] = {0, 0};
            const uint32_t *ok = nullptr, *ds = nullptr;
            if (rc == 0 && n) rc = mcx_batch_sums(c, &nc, &ok, &ds, nullptr);
            if (rc == 0 && n) rc = mcx_batch_totals(c, tot);
            mine.rc = (uint32_t)rc; mine.n_chunks = rc ? 0 : nc; mine.n_redo = n_redo; mine.pad = 0; mine.pairs = tot[0]; mine.dist = tot[1];
            if (int e = gather(&mine, sizeof mine)) return e;
            bool settled = iter > 0;
            int64_t before[3] = {avg[0], avg[1], avg[2]}, all_pairs = 0, all_dist = 0, all_chunks = 0;
            bool first = true; // no shard before this one holds a chunk
            for (int r = 0; r < x->size; r++) {
                memcpy(&o, recv.data() + (size_t)r * sizeof o, sizeof o);
                if (o.rc) return rc ? rc : mcx_set_error((int32_t)o.rc, "shard " + std::to_string(r) + " failed");
                if (o.n_chunks && o.n_redo) settled = false;
                if (r < x->rank) { before[1] += o.pairs; before[2] += o.dist; if (o.n_chunks) first = false; }
                all_pairs += o.pairs; all_dist += o.dist; all_chunks += o.n_chunks;
            }
            st[0] = avg[0]; st[1] = avg[1]; st[2] = avg[2];
            mcx_avg_advance(st, all_pairs, all_dist, all_chunks);
            if (settled) break;
            if (iter == 255) return mcx_set_error(MCX_ERR_CAPACITY, "avgDist replay did not converge");
            n_redo = 0;
            if (n) {
                // this shard's chunks walked HERE, from the round's state plus the totals of the shards before it (ReadMapping.cpp:462, :538-539): the
                // estimate a chunk is paired with is the state before it, re-estimated once a thousand proper pairs have been seen — not at the round's
                // very first chunk, whose estimate is the state the round began with.  The device checks every pair against the list and re-runs the
                // ones whose estimate moved (mcx_batch_replay).  (Round 5 left the walk to the device here — mcx_batch_check, closed form — with nothing
                // on the host to hold it against; the one-shard path has always compared the two.)
                est.resize(nc);
                uint32_t cur = (uint32_t)before[0];
                int64_t tp = before[1], td = before[2];
                for (uint32_t k = 0; k < nc; k++) {
                    if ((k > 0 || !first) && tp > 1000) cur = (uint32_t)(int)(1. * td / tp + .5);
                    est[k] = (int32_t)(cur * 1.5);
                    tp += ok[k]; td += ds[k];
                }
                rc = mcx_batch_replay(c, est.data(), &n_redo, stats);
            }
        }
        avg[0] = st[0]; avg[1] = st[1]; avg[2] = st[2];
        return finish_part(c, n != 0, profile, stats, 0);
    }

    // reads mapped one by one (single-end libraries, the odd tail of an interleaved file): no trajectory
    int singles(mcx_ctx *c, const uint8_t *d_bases, const uint32_t *d_off, uint32_t n, int64_t read_base, bool profile, mcx_aln *d_aln, uint32_t *d_cig,
                mcx_stats *stats)
    {
        int rc = 0;
        if (n) rc = mcx_batch_begin(c, d_bases, d_off, n, 0, 0, read_base, d_aln, d_cig, stats);
        return finish_part(c, n != 0 && rc == 0, profile, stats, rc);
    }
};

// what the formatter and the thread that talks to the other shards tell each other: sizes one way, places the other
struct Places {
    std::mutex m; std::condition_variable cv;
    std::map<uint64_t, uint64_t> size, place; // batch number -> bytes of its text; -> where it goes
    bool failed = false;
    void put_size(uint64_t k, uint64_t v) { std::unique_lock<std::mutex> l(m); size[k] = v; cv.notify_all(); }
    bool wait_size(uint64_t k, uint64_t &v) // false: the run has failed, there is no such size
    {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return failed || size.count(k); });
        if (!size.count(k)) return false;
        v = size[k]; size.erase(k);
        return true;
    }
    void put_place(uint64_t k, uint64_t v) { std::unique_lock<std::mutex> l(m); place[k] = v; cv.notify_all(); }
    // the place of batch k, or of nothing at all when the run has failed (false)
    bool wait_place(uint64_t k, uint64_t &v, bool block)
    {
        std::unique_lock<std::mutex> l(m);
        if (block) cv.wait(l, [&] { return failed || place.count(k); });
        auto it = place.find(k);
        if (it == place.end()) return false;
        v = it->second; place.erase(it);
        return true;
    }
    void fail() { std::unique_lock<std::mutex> l(m); failed = true; cv.notify_all(); }
    bool has_failed() { std::unique_lock<std::mutex> l(m); return failed; }
};

}} // namespace mcx::files
