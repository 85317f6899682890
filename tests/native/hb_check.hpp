// tests/native/hb_check.hpp — happens-before checker over a trace of stream operations.
//
// A trace is the total host order in which operations were ISSUED (tests/native/fake_hip.cpp appends under one
// mutex).  From it the checker builds the order the device is bound to keep, by HIP's rules:
//   stream order   items of one stream run in issue order;
//   event edges    hipStreamWaitEvent(s, e) puts everything behind it on s after the LATEST hipEventRecord(e) that
//                  precedes the wait call in host order; without such a record the wait is a no-op;
//   host syncs     what a synchronising call covers (a stream, an event's record, the device) happens before every
//                  item issued later in host order, BY ANY THREAD.  Across threads this is deliberately generous:
//                  it assumes the later thread learnt of the sync (a barrier, a channel), which is what the
//                  barrier-synchronised direct collectives do.  The checker therefore cannot report a false hazard
//                  there, and can miss a real one: the direct paths' host ordering stays with TSan and the GPU
//                  suite; the event-ordered paths (ring, Rabenseifner, staged, grouped) are this checker's target.
// and reports every pair of operations whose byte ranges intersect, of which at least one writes, and which that
// order leaves unordered: under some schedule HIP allows, the two run concurrently or in the wrong order.
//
// Every edge above points forward in host order, so the relation is acyclic by construction.  The cycle report
// therefore asks a second question: would the streams deadlock under a runtime (or a reader) that binds a wait to
// the NEXT record when none precedes it?  A wait that precedes its record in host order is reported as unbound,
// and for the cycle search alone it is bound to the first later record of its event.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <string>
#include <vector>

namespace hb {

struct Range {
    uintptr_t lo = 0, hi = 0;  // [lo, hi)
    bool write = false;        // a read-modify-write is a write
};

enum class Kind { kOp, kRecord, kWait, kSync };
enum class Covers { kStream, kEvent, kDevice };  // what a kSync waits for

// Streams and events are ids.  A call site is (rank, call index, entry point or HIP function); the scenario is the
// trace's.
struct Rec {
    Kind kind = Kind::kOp;
    uint64_t stream = 0;  // kOp / kRecord / kWait: where it is enqueued; kSync + kStream: what it drains
    uint64_t event = 0;   // kRecord / kWait; kSync + kEvent
    Covers covers = Covers::kStream;
    std::vector<Range> ranges;  // kOp
    std::string fn;
    int rank = -1, call = -1;
    bool user = false;  // a synthetic operation of the harness (producer / consumer / clobber), not library work
};
using Trace = std::vector<Rec>;

struct Hazard {
    size_t a = 0, b = 0;  // trace indices, a < b
    bool operator==(const Hazard& o) const { return a == o.a && b == o.b; }
};

struct Report {
    std::vector<Hazard> hazards;
    std::vector<size_t> unbound_waits;        // waits with no earlier record of their event but a later one
    std::vector<std::vector<size_t>> cycles;  // each: the trace indices around one cycle (late binding, see above)
    size_t ops = 0, waits = 0;
};

inline bool conflict(const Rec& x, const Rec& y) {
    for (const Range& p : x.ranges)
        for (const Range& q : y.ranges)
            if ((p.write || q.write) && p.lo < q.hi && q.lo < p.hi) return true;
    return false;
}

class Checker {
public:
    explicit Checker(const Trace& t) : t_(t), n_(t.size()), words_((t.size() + 63) / 64) {
        // Conflicting pairs do not depend on which waits count: find them once.  Same-stream pairs are ordered.
        std::vector<size_t> ops;
        for (size_t i = 0; i < n_; ++i)
            if (t_[i].kind == Kind::kOp && !t_[i].ranges.empty()) ops.push_back(i);
        for (size_t x = 0; x < ops.size(); ++x)
            for (size_t y = x + 1; y < ops.size(); ++y)
                if (t_[ops[x]].stream != t_[ops[y]].stream && conflict(t_[ops[x]], t_[ops[y]]))
                    pairs_.push_back(Hazard{ops[x], ops[y]});
        for (size_t i = 0; i < n_; ++i) {
            if (t_[i].kind == Kind::kOp) ++n_ops_;
            if (t_[i].kind == Kind::kWait) waits_.push_back(i);
        }
    }

    const std::vector<size_t>& waits() const { return waits_; }

    // The report with the waits in `ignored` (trace indices) treated as absent.
    Report analyse(const std::set<size_t>& ignored = {}) const {
        Report rep;
        rep.ops = n_ops_;
        rep.waits = waits_.size();
        std::vector<std::vector<size_t>> preds(n_);
        std::map<uint64_t, size_t> last_on_stream, latest_record;
        std::vector<std::pair<size_t, size_t>> late;  // (record, wait) edges of the late binding
        size_t last_sync = n_;
        for (size_t i = 0; i < n_; ++i) {
            const Rec& r = t_[i];
            if (r.kind == Kind::kSync) {
                if (r.covers == Covers::kStream) {
                    const auto it = last_on_stream.find(r.stream);
                    if (it != last_on_stream.end()) preds[i].push_back(it->second);
                } else if (r.covers == Covers::kEvent) {
                    const auto it = latest_record.find(r.event);
                    if (it != latest_record.end()) preds[i].push_back(it->second);
                } else {
                    for (const auto& kv : last_on_stream) preds[i].push_back(kv.second);
                }
                if (last_sync != n_) preds[i].push_back(last_sync);
                last_sync = i;
                continue;
            }
            const auto prev = last_on_stream.find(r.stream);
            if (prev != last_on_stream.end()) preds[i].push_back(prev->second);
            last_on_stream[r.stream] = i;
            if (last_sync != n_) preds[i].push_back(last_sync);
            if (r.kind == Kind::kRecord) latest_record[r.event] = i;
            if (r.kind == Kind::kWait && ignored.count(i) == 0) {
                const auto rec = latest_record.find(r.event);
                if (rec != latest_record.end()) {
                    preds[i].push_back(rec->second);
                } else {
                    for (size_t j = i + 1; j < n_; ++j)
                        if (t_[j].kind == Kind::kRecord && t_[j].event == r.event) {
                            rep.unbound_waits.push_back(i);
                            late.emplace_back(j, i);
                            break;
                        }
                }
            }
        }
        // ancestors, in host order (a topological order: every edge points forward)
        std::vector<uint64_t> anc(n_ * words_, 0);
        for (size_t i = 0; i < n_; ++i) {
            uint64_t* mine = &anc[i * words_];
            for (size_t p : preds[i]) {
                const uint64_t* theirs = &anc[p * words_];
                for (size_t w = 0; w <= p / 64; ++w) mine[w] |= theirs[w];
                mine[p / 64] |= uint64_t(1) << (p % 64);
            }
        }
        for (const Hazard& h : pairs_)
            if (((anc[h.b * words_ + h.a / 64] >> (h.a % 64)) & 1) == 0) rep.hazards.push_back(h);
        if (!late.empty()) find_cycles(preds, late, &rep);
        return rep;
    }

private:
    // Depth-first search over successor lists with the late-bound edges added; every back edge closes one cycle.
    void find_cycles(const std::vector<std::vector<size_t>>& preds, const std::vector<std::pair<size_t, size_t>>& late,
                     Report* rep) const {
        std::vector<std::vector<size_t>> succ(n_);
        for (size_t i = 0; i < n_; ++i)
            for (size_t p : preds[i]) succ[p].push_back(i);
        for (const auto& e : late) succ[e.first].push_back(e.second);
        std::vector<int> colour(n_, 0);  // 0 new, 1 on the path, 2 done
        std::vector<size_t> path, next(n_, 0);
        for (size_t root = 0; root < n_; ++root) {
            if (colour[root] != 0) continue;
            path.push_back(root);
            colour[root] = 1;
            while (!path.empty()) {
                const size_t v = path.back();
                if (next[v] == succ[v].size()) {
                    colour[v] = 2;
                    path.pop_back();
                    continue;
                }
                const size_t w = succ[v][next[v]++];
                if (colour[w] == 0) {
                    colour[w] = 1;
                    path.push_back(w);
                } else if (colour[w] == 1 && rep->cycles.size() < 8) {
                    const auto at = std::find(path.begin(), path.end(), w);
                    rep->cycles.emplace_back(at, path.end());
                }
            }
        }
    }

    const Trace& t_;
    size_t n_, words_, n_ops_ = 0;
    std::vector<Hazard> pairs_;
    std::vector<size_t> waits_;
};

// The waits without which a hazard appears that the whole trace does not have: each ignored alone.
inline std::vector<size_t> load_bearing_waits(const Checker& c) {
    std::vector<size_t> out;
    const size_t base = c.analyse().hazards.size();
    for (size_t w : c.waits())
        if (c.analyse({w}).hazards.size() > base) out.push_back(w);
    return out;
}

}  // namespace hb
