// tests/native/stream_order_harness.cpp — the collectives' stream ordering, checked on the CPU.
//
// Links the host code of the collectives (comm.cpp, algorithms.cpp, grouped.cpp, bootstrap.cpp, dccl_api.cpp,
// direct.cpp, rccl_transport.cpp) against the recording fake runtime (fake_hip.cpp) and runs scenarios on W thread
// ranks through the public dccl:: API, every rank on non-default fake streams.  Around every call the harness
// enqueues synthetic user operations on the call's own stream: before it a PRODUCER that writes sendbuff (and
// recvbuff for an accumulating sum), after it a CONSUMER that reads recvbuff and a CLOBBER that writes sendbuff.
// Library work on a wrong stream, or a peer still reading a buffer in place after the call returned, then shows as
// a hazard against user memory; library scratch reused too early shows as a hazard between two library operations.
// tests/native/hb_check.hpp decides what is ordered.  Per scenario the harness also checks that the library wrote
// exactly recvbuff (nothing on a non-root rank of ncclReduce; the bytes an in-place call already holds may stay
// untouched) and read user memory only inside sendbuff, recvbuff or a device scalar.
//
// Output: one JSON line per hand-written self-check trace, one per scenario, one summary.  tests/test_stream_order.py
// asserts on them.  Exit status 0 unless the harness itself failed.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "comm.hpp"
#include "dccl/dccl.hpp"
#include "fake_hip.hpp"
#include "hb_check.hpp"

namespace {

using dccl::ncclResult_t;

enum Api { kAR, kRS, kRED, kAG, kBC };
enum OpKind { kSum, kPremulHost, kPremulDev, kWide, kScaledHost, kScaledDev, kWidened0, kWidened1 };

// One collective call.  `n` counts the elements of the whole buffer the collective works on: count for
// ncclAllReduce / ncclReduce / ncclBroadcast, W * recvcount for ncclReduceScatter, W * sendcount for ncclAllGather.
struct Spec {
    Api api = kAR;
    OpKind op = kSum;
    size_t n = 0;
    int root = 0;
    bool in_place = false;
};

struct Item {
    Spec spec;
    int buf = 0;     // which of the rank's buffer sets the call uses: calls that share one reuse the same memory
    int stream = 0;  // which of the rank's streams
};

struct Phase {
    bool grouped = false;  // inside ncclGroupStart / ncclGroupEnd
    std::vector<Item> items;
};

struct Scenario {
    std::string name;
    uint32_t W = 1;
    std::map<std::string, std::string> env;
    std::vector<Phase> phases;
    bool event_ordered = false;  // every path in it orders by events (no host sync): it must have load-bearing waits
};

bool widened(OpKind k) { return k == kWidened0 || k == kWidened1; }
bool sixteen(OpKind k) { return k == kWide || k == kScaledHost || k == kScaledDev || widened(k); }

struct Bufs {
    void* send = nullptr;
    size_t send_bytes = 0;
    void* recv = nullptr;
    size_t recv_bytes = 0;
    uintptr_t keep_lo = 0, keep_hi = 0;  // bytes of recvbuff an in-place call may leave as they are
};

void* dev_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) std::abort();
    return p;
}

Bufs make_bufs(const Spec& s, uint32_t W, uint32_t r) {
    const size_t esz = sixteen(s.op) ? 2 : 4, out = widened(s.op) ? 4 : esz;
    const bool root = r == uint32_t(s.root);
    Bufs b;
    switch (s.api) {
    case kAR:
        b.send_bytes = b.recv_bytes = s.n * esz;
        b.send = dev_alloc(b.send_bytes);
        b.recv = s.in_place ? b.send : dev_alloc(b.recv_bytes);
        break;
    case kRS:
        b.send_bytes = s.n * esz;
        b.recv_bytes = s.n / W * out;
        b.send = dev_alloc(b.send_bytes);
        b.recv = s.in_place ? static_cast<unsigned char*>(b.send) + r * b.recv_bytes : dev_alloc(b.recv_bytes);
        break;
    case kRED:
        b.send_bytes = s.n * esz;
        b.send = dev_alloc(b.send_bytes);
        if (root) {
            b.recv_bytes = s.n * out;
            b.recv = s.in_place ? b.send : dev_alloc(b.recv_bytes);
        }
        break;
    case kAG:
        b.send_bytes = s.n / W * esz;
        b.recv_bytes = s.n * esz;
        b.recv = dev_alloc(b.recv_bytes);
        b.send = s.in_place ? static_cast<unsigned char*>(b.recv) + r * b.send_bytes : dev_alloc(b.send_bytes);
        if (s.in_place) b.keep_lo = reinterpret_cast<uintptr_t>(b.send), b.keep_hi = b.keep_lo + b.send_bytes;
        break;
    case kBC:
        b.recv_bytes = s.n * esz;
        b.recv = dev_alloc(b.recv_bytes);
        if (root) {
            b.send_bytes = s.n * esz;
            b.send = s.in_place ? b.recv : dev_alloc(b.send_bytes);
            if (s.in_place) b.keep_lo = reinterpret_cast<uintptr_t>(b.recv), b.keep_hi = b.keep_lo + b.recv_bytes;
        } else if (s.in_place) {
            b.send = b.recv;  // ncclBcast passes one buffer on every rank; a non-root's is only written
        }
        break;
    }
    // W = 1, in place, a sum that leaves the input's bytes (plain or wide): the result is already there, and the
    // library rightly launches nothing.  (A pre-multiplied or scaled sum still multiplies in place.)
    if (W == 1 && s.in_place && s.api <= kRED && (s.op == kSum || s.op == kWide))
        b.keep_lo = reinterpret_cast<uintptr_t>(b.recv), b.keep_hi = b.keep_lo + b.recv_bytes;
    return b;
}

// What one rank keeps for a scenario.
struct RankCtx {
    uint32_t W = 1, r = 0;
    dccl::ncclComm_t comm = nullptr;
    std::vector<hipStream_t> streams;
    std::map<int, Bufs> bufs;
    std::map<int, dccl::ncclRedOp_t> ops;
    float host_scalar = 0.5f;
    void* dev_scalar = nullptr;
    ncclResult_t first = dccl::ncclSuccess;
    void keep(ncclResult_t rc) {
        if (first == dccl::ncclSuccess) first = rc;
    }
};

dccl::ncclRedOp_t op_of(RankCtx& c, OpKind k) {
    if (k == kSum) return dccl::ncclSum;
    const auto it = c.ops.find(k);
    if (it != c.ops.end()) return it->second;
    dccl::ncclRedOp_t op = dccl::ncclSum;
    const bool device = k == kPremulDev || k == kScaledDev;
    if (device && c.dev_scalar == nullptr) c.dev_scalar = dev_alloc(8);
    void* scalar = device ? c.dev_scalar : static_cast<void*>(&c.host_scalar);
    const auto res = device ? dccl::ncclScalarDevice : dccl::ncclScalarHostImmediate;
    switch (k) {
    case kPremulHost:
    case kPremulDev: c.keep(dccl::ncclRedOpCreatePreMulSum(&op, scalar, dccl::ncclFloat32, res, c.comm)); break;
    case kWide: c.keep(dccl::dcclRedOpCreateWideSum(&op, dccl::ncclBfloat16, c.comm)); break;
    case kScaledHost:
    case kScaledDev: c.keep(dccl::dcclRedOpCreateWideScaledSum(&op, scalar, dccl::ncclBfloat16, res, c.comm)); break;
    case kWidened0: c.keep(dccl::dcclRedOpCreateWidenedSum(&op, dccl::ncclBfloat16, 0, c.comm)); break;
    case kWidened1: c.keep(dccl::dcclRedOpCreateWidenedSum(&op, dccl::ncclBfloat16, 1, c.comm)); break;
    case kSum: break;
    }
    c.ops[k] = op;
    return op;
}

const Bufs& bufs_of(RankCtx& c, const Item& it) {
    auto at = c.bufs.find(it.buf);
    if (at == c.bufs.end()) at = c.bufs.emplace(it.buf, make_bufs(it.spec, c.W, c.r)).first;
    return at->second;
}

void producer(RankCtx& c, const Item& it) {
    const Bufs& b = bufs_of(c, it);
    std::vector<hb::Range> w;
    if (b.send_bytes != 0 && !(it.spec.api == kBC && c.r != uint32_t(it.spec.root)))
        w.push_back(fake::writes(b.send, b.send_bytes));
    if (it.spec.op == kWidened1 && b.recv_bytes != 0) w.push_back(fake::writes(b.recv, b.recv_bytes));
    if (!w.empty()) fake::user_op(c.streams[it.stream], "producer", std::move(w));
}

void consumer_and_clobber(RankCtx& c, const Item& it) {
    const Bufs& b = bufs_of(c, it);
    hipStream_t st = c.streams[it.stream];
    if (b.recv_bytes != 0) fake::user_op(st, "consumer", {fake::reads(b.recv, b.recv_bytes)});
    if (b.send_bytes != 0) fake::user_op(st, "clobber", {fake::writes(b.send, b.send_bytes)});
}

ncclResult_t issue(RankCtx& c, const Item& it) {
    const Spec& s = it.spec;
    const Bufs& b = bufs_of(c, it);
    hipStream_t st = c.streams[it.stream];
    const auto dt = sixteen(s.op) ? dccl::ncclBfloat16 : dccl::ncclFloat32;
    const dccl::ncclRedOp_t op = s.api <= kRED ? op_of(c, s.op) : dccl::ncclSum;
    switch (s.api) {
    case kAR: return dccl::ncclAllReduce(b.send, b.recv, s.n, dt, op, c.comm, st);
    case kRS: return dccl::ncclReduceScatter(b.send, b.recv, s.n / c.W, dt, op, c.comm, st);
    case kRED: return dccl::ncclReduce(b.send, b.recv, s.n, dt, op, s.root, c.comm, st);
    case kAG: return dccl::ncclAllGather(b.send, b.recv, s.n / c.W, dt, c.comm, st);
    case kBC: return dccl::ncclBroadcast(b.send, b.recv, s.n, dt, s.root, c.comm, st);
    }
    return dccl::ncclInternalError;
}

// Which of the communicator's events an id is, for the load-bearing table.
std::mutex g_class_mu;
std::map<uint64_t, std::string> g_event_class;

void classify_events(const dccl::dcclComm* comm) {
    std::lock_guard<std::mutex> lk(g_class_mu);
    auto put = [](hipEvent_t e, const char* what) {
        if (e != nullptr) g_event_class[reinterpret_cast<uintptr_t>(e)] = what;
    };
    for (hipEvent_t e : comm->ready_events) put(e, "ready");
    for (hipEvent_t e : comm->done_events) put(e, "done");
    put(comm->dev_pack_done, "pack_done");
    put(comm->dev_pack_join, "pack_join");
    put(comm->dev_scratch_done, "scratch_done");
}

struct RankOut {
    ncclResult_t rc = dccl::ncclSuccess;
    std::map<int, Bufs> bufs;
    uintptr_t scalar = 0;
};

void rank_main(const Scenario& sc, uint32_t r, RankOut* out) {
    RankCtx c;
    c.W = sc.W;
    c.r = r;
    fake::set_site(int(r), -1);
    c.keep(dccl::dcclCommInitRank(&c.comm, sc.W, r));
    if (c.comm == nullptr) {
        out->rc = c.first;
        return;
    }
    for (int i = 0; i < 3; ++i) c.streams.push_back(fake::new_stream());
    int call = 0;
    for (const Phase& ph : sc.phases) {
        if (!ph.grouped) {
            for (const Item& it : ph.items) {
                fake::set_site(int(r), call++);
                producer(c, it);
                c.keep(issue(c, it));
                consumer_and_clobber(c, it);
            }
            continue;
        }
        fake::set_site(int(r), call++);  // the whole group is one call site: its collectives run at ncclGroupEnd
        for (const Item& it : ph.items) producer(c, it);
        c.keep(dccl::ncclGroupStart());
        for (const Item& it : ph.items) c.keep(issue(c, it));
        c.keep(dccl::ncclGroupEnd());
        for (const Item& it : ph.items) consumer_and_clobber(c, it);
    }
    fake::set_site(int(r), -1);
    // Every rank's operations are in the trace before any rank finalises: ncclCommFinalize synchronises the device,
    // and the checker lets a host synchronisation order everything issued after it, by any thread.
    c.comm->group->barrier();
    classify_events(c.comm);
    for (const auto& kv : c.ops) c.keep(dccl::ncclRedOpDestroy(kv.second, c.comm));
    c.keep(dccl::ncclCommFinalize(c.comm));
    out->rc = c.first;
    out->bufs = c.bufs;
    out->scalar = reinterpret_cast<uintptr_t>(c.dev_scalar);
}

// ----------------------------------------------------------------------------------------------- byte checks
using Intervals = std::vector<std::pair<uintptr_t, uintptr_t>>;

Intervals merged(Intervals v) {
    std::sort(v.begin(), v.end());
    Intervals out;
    for (const auto& x : v) {
        if (x.first >= x.second) continue;
        if (!out.empty() && x.first <= out.back().second) out.back().second = std::max(out.back().second, x.second);
        else out.push_back(x);
    }
    return out;
}

bool covered(const Intervals& m, uintptr_t lo, uintptr_t hi) {  // [lo, hi) inside one merged interval
    for (const auto& x : m)
        if (x.first <= lo && hi <= x.second) return true;
    return lo >= hi;
}

// The library wrote exactly recvbuff (minus what an in-place call may keep) and read user memory only inside
// sendbuff, recvbuff or a device scalar.
std::vector<std::string> check_bytes(const hb::Trace& t, const std::vector<RankOut>& outs) {
    std::vector<std::string> errors;
    Intervals user, readable, must_write, may_write;
    for (const RankOut& o : outs) {
        if (o.scalar != 0) {
            user.emplace_back(o.scalar, o.scalar + 8);
            readable.emplace_back(o.scalar, o.scalar + 8);
        }
        for (const auto& kv : o.bufs) {
            const Bufs& b = kv.second;
            const uintptr_t s = reinterpret_cast<uintptr_t>(b.send), v = reinterpret_cast<uintptr_t>(b.recv);
            if (b.send_bytes != 0) user.emplace_back(s, s + b.send_bytes), readable.emplace_back(s, s + b.send_bytes);
            if (b.recv_bytes == 0) continue;
            user.emplace_back(v, v + b.recv_bytes);
            readable.emplace_back(v, v + b.recv_bytes);
            may_write.emplace_back(v, v + b.recv_bytes);
            if (b.keep_lo == b.keep_hi) {
                must_write.emplace_back(v, v + b.recv_bytes);
            } else {
                must_write.emplace_back(v, b.keep_lo);
                must_write.emplace_back(b.keep_hi, v + b.recv_bytes);
            }
        }
    }
    user = merged(user), readable = merged(readable), may_write = merged(may_write);
    Intervals written;
    auto in_user = [&](const hb::Range& g) {
        for (const auto& u : user)
            if (g.lo < u.second && u.first < g.hi) return true;
        return false;
    };
    for (const hb::Rec& rec : t) {
        if (rec.kind != hb::Kind::kOp || rec.user) continue;
        for (const hb::Range& g : rec.ranges) {
            if (!in_user(g)) continue;
            const Intervals& allowed = g.write ? may_write : readable;
            if (!covered(allowed, g.lo, g.hi))
                errors.push_back(std::string(g.write ? "write" : "read") + " outside the call's buffers by " + rec.fn +
                                 " rank " + std::to_string(rec.rank) + " call " + std::to_string(rec.call));
            if (g.write) written.emplace_back(g.lo, g.hi);
        }
    }
    written = merged(written);
    for (const auto& m : merged(must_write))
        if (!covered(written, m.first, m.second)) errors.push_back("recvbuff bytes the library never wrote");
    return errors;
}

// ------------------------------------------------------------------------------------------------- reporting
std::string site(const hb::Rec& r, const std::string& scenario) {
    return "{\"scenario\": \"" + scenario + "\", \"rank\": " + std::to_string(r.rank) + ", \"call\": " +
           std::to_string(r.call) + ", \"fn\": \"" + r.fn + "\", \"user\": " + (r.user ? "true" : "false") + "}";
}

std::string wait_class(const hb::Trace& t, size_t w) {
    const auto it = g_event_class.find(t[w].event);
    std::string cls = it == g_event_class.end() ? "other" : it->second;
    if (cls != "pack_join") return cls;
    // a join INTO the run's stream is a wait on the stream the pack / unpack kernels of that group run on
    for (const hb::Rec& r : t)
        if (r.kind == hb::Kind::kOp && r.rank == t[w].rank && r.call == t[w].call && r.stream == t[w].stream &&
            (r.fn == "copy_rows_launch" || r.fn == "add_rows_launch"))
            return "join_in";
    return "join_out";
}

int g_failed_scenarios = 0;

void run_scenario(const Scenario& sc) {
    fake::reset();
    {
        std::lock_guard<std::mutex> lk(g_class_mu);
        g_event_class.clear();
    }
    for (const char* k : {"DCCL_ALLREDUCE_ALGORITHM", "DCCL_RS_SCRATCH", "DCCL_GROUP_COALESCE",
                          "DCCL_GROUP_COALESCE_MAX_BYTES", "DCCL_FAULT_INJECT", "DCCL_TRANSPORT"})
        unsetenv(k);
    for (const auto& kv : sc.env) setenv(kv.first.c_str(), kv.second.c_str(), 1);
    std::vector<RankOut> outs(sc.W);
    std::vector<std::thread> threads;
    for (uint32_t r = 0; r < sc.W; ++r) threads.emplace_back(rank_main, std::cref(sc), r, &outs[r]);
    for (std::thread& th : threads) th.join();
    const hb::Trace t = fake::trace();
    const hb::Checker chk(t);
    const hb::Report rep = chk.analyse();
    const std::vector<std::string> bytes = check_bytes(t, outs);
    std::map<std::string, std::pair<size_t, size_t>> by_class;  // (load-bearing, total)
    for (size_t w : chk.waits()) ++by_class[wait_class(t, w)].second;
    size_t lb_total = 0;
    for (size_t w : hb::load_bearing_waits(chk)) ++by_class[wait_class(t, w)].first, ++lb_total;
    // every wait of one class ignored together: the hazards that class as a whole keeps away (one wait alone may be
    // covered by the same class's waits on other ranks)
    std::map<std::string, size_t> without_class;
    for (const auto& kv : by_class) {
        std::set<size_t> all;
        for (size_t w : chk.waits())
            if (wait_class(t, w) == kv.first) all.insert(w);
        without_class[kv.first] = chk.analyse(all).hazards.size();
    }
    bool rc_ok = true;
    std::string line = "{\"scenario\": \"" + sc.name + "\", \"W\": " + std::to_string(sc.W) + ", \"rc\": [";
    for (uint32_t r = 0; r < sc.W; ++r) {
        line += (r ? ", " : "") + std::to_string(int(outs[r].rc));
        rc_ok = rc_ok && outs[r].rc == dccl::ncclSuccess;
    }
    line += "], \"ops\": " + std::to_string(rep.ops) + ", \"waits\": " + std::to_string(rep.waits) + ", \"hazards\": [";
    for (size_t i = 0; i < rep.hazards.size() && i < 16; ++i)
        line += std::string(i ? ", " : "") + "{\"a\": " + site(t[rep.hazards[i].a], sc.name) + ", \"b\": " +
                site(t[rep.hazards[i].b], sc.name) + "}";
    line += "], \"n_hazards\": " + std::to_string(rep.hazards.size()) + ", \"cycles\": " +
            std::to_string(rep.cycles.size()) + ", \"unbound_waits\": " + std::to_string(rep.unbound_waits.size()) +
            ", \"bytes_errors\": [";
    for (size_t i = 0; i < bytes.size() && i < 8; ++i) line += std::string(i ? ", " : "") + "\"" + bytes[i] + "\"";
    line += std::string("], \"event_ordered\": ") + (sc.event_ordered ? "true" : "false") + ", \"load_bearing\": {";
    bool first = true;
    for (const auto& kv : by_class) {
        line += std::string(first ? "" : ", ") + "\"" + kv.first + "\": [" + std::to_string(kv.second.first) + ", " +
                std::to_string(kv.second.second) + "]";
        first = false;
    }
    line += "}, \"hazards_without_class\": {";
    first = true;
    for (const auto& kv : without_class) {
        line += std::string(first ? "" : ", ") + "\"" + kv.first + "\": " + std::to_string(kv.second);
        first = false;
    }
    line += "}, \"load_bearing_total\": " + std::to_string(lb_total) + "}";
    std::puts(line.c_str());
    if (!rc_ok || !rep.hazards.empty() || !rep.cycles.empty() || !bytes.empty()) ++g_failed_scenarios;
}

// ------------------------------------------------------------------------------------------------- scenarios
Item item(Api api, OpKind op, size_t n, int root = 0, bool in_place = false, int buf = 0, int stream = 0) {
    Item it;
    it.spec.api = api, it.spec.op = op, it.spec.n = n, it.spec.root = root, it.spec.in_place = in_place;
    it.buf = buf, it.stream = stream;
    return it;
}

using Env = std::map<std::string, std::string>;

std::vector<Scenario> g_scenarios;

const char* api_name(Api a) {
    static const char* names[] = {"all_reduce", "reduce_scatter", "reduce", "all_gather", "broadcast"};
    return names[a];
}
const char* op_name(OpKind k) {
    static const char* names[] = {"sum", "premul_host", "premul_dev", "wide", "scaled_host", "scaled_dev",
                                  "widened_acc0", "widened_acc1"};
    return names[k];
}

// One call alone (A / B), and the same call three times on one stream and one set of buffers with no host
// synchronisation in between (C): that wraps the W - 1 event ring.
void add_single_and_thrice(const std::string& path, uint32_t W, const Env& env, const Item& it, bool event_ordered) {
    const std::string base = std::string(api_name(it.spec.api)) + "/" + path + "/W" + std::to_string(W) + "/" +
                             op_name(it.spec.op) + "/n" + std::to_string(it.spec.n) + "/root" +
                             std::to_string(it.spec.root) + (it.spec.in_place ? "/in_place" : "/out_of_place");
    Scenario one;
    one.name = "single/" + base;
    one.W = W;
    one.env = env;
    one.event_ordered = event_ordered && W > 1;
    one.phases.push_back(Phase{false, {it}});
    g_scenarios.push_back(one);
    Scenario three = one;
    three.name = "thrice/" + base;
    three.event_ordered = event_ordered && W > 1;
    three.phases = {Phase{false, {it, it, it}}};
    g_scenarios.push_back(three);
}

// Two calls of one communicator on two different streams, each with buffers of its own, no host synchronisation.
void add_pair(const std::string& what, uint32_t W, const Env& env, Item a, Item b) {
    a.buf = 0, a.stream = 0, b.buf = 1, b.stream = 1;
    Scenario sc;
    sc.name = "two_streams/" + what + "/W" + std::to_string(W);
    sc.W = W;
    sc.env = env;
    sc.event_ordered = true;
    sc.phases = {Phase{false, {a, b}}};
    g_scenarios.push_back(sc);
}

void build_scenarios() {
    const Env direct{{"DCCL_ALLREDUCE_ALGORITHM", ""}}, ring{{"DCCL_ALLREDUCE_ALGORITHM", "ring"}},
        rab{{"DCCL_ALLREDUCE_ALGORITHM", "rabenseifner"}},
        ring_pad{{"DCCL_ALLREDUCE_ALGORITHM", "ring"}, {"DCCL_RS_SCRATCH", "1"}},
        rab_pad{{"DCCL_ALLREDUCE_ALGORITHM", "rabenseifner"}, {"DCCL_RS_SCRATCH", "1"}};
    auto sizes = [](uint32_t W) { return std::vector<size_t>{size_t(W) * 8, size_t(W) * 1031}; };
    // A: every API on every path select() gives the thread transport.
    for (uint32_t W : {2u, 3u, 4u})
        for (size_t n : sizes(W))
            for (bool ip : {false, true}) add_single_and_thrice("ring", W, ring, item(kAR, kSum, n, 0, ip), true);
    for (uint32_t W : {4u, 5u})
        for (size_t n : {size_t(W) * 8, size_t(4) * 1031})  // Rabenseifner cuts into 4 slots at both sizes
            for (bool ip : {false, true}) add_single_and_thrice("rabenseifner", W, rab, item(kAR, kSum, n, 0, ip), true);
    for (bool ip : {false, true}) {
        add_single_and_thrice("ring_scratchpad", 3, ring_pad, item(kAR, kSum, 3 * 1031, 0, ip), true);
        add_single_and_thrice("rabenseifner_scratchpad", 4, rab_pad, item(kAR, kSum, 4 * 1031, 0, ip), true);
    }
    for (size_t n : sizes(3))
        for (bool ip : {false, true}) {
            add_single_and_thrice("direct", 3, direct, item(kAR, kSum, n, 0, ip), false);
            add_single_and_thrice("ring", 3, ring, item(kRS, kSum, n, 0, ip), true);
            add_single_and_thrice("ring_scratchpad", 3, ring_pad, item(kRS, kSum, n, 0, ip), true);
            add_single_and_thrice("direct", 3, direct, item(kRS, kSum, n, 0, ip), false);
            add_single_and_thrice("ring", 3, ring, item(kAG, kSum, n, 0, ip), true);
            add_single_and_thrice("direct", 3, direct, item(kAG, kSum, n, 0, ip), false);
            for (int root : {0, 1}) {
                add_single_and_thrice("ring_gather", 3, ring, item(kRED, kSum, n, root, ip), true);
                add_single_and_thrice("direct", 3, direct, item(kRED, kSum, n, root, ip), false);
                add_single_and_thrice("fan_out", 3, ring, item(kBC, kSum, n, root, ip), true);
                add_single_and_thrice("direct", 3, direct, item(kBC, kSum, n, root, ip), false);
            }
        }
    // W = 9 is above kDirectMaxWorld: the unnamed algorithm is the ring
    add_single_and_thrice("auto_above_direct", 9, direct, item(kAR, kSum, 9 * 8), true);
    add_single_and_thrice("auto_above_direct", 9, direct, item(kRS, kSum, 9 * 8), true);
    // B: every SumKind on its staged route, W = 1 and W = 3.
    for (uint32_t W : {1u, 3u})
        for (size_t n : {size_t(W) * 8, size_t(W) * 1031}) {
            for (OpKind k : {kPremulHost, kPremulDev}) {
                add_single_and_thrice("ring", W, ring, item(kAR, k, n), true);
                add_single_and_thrice("ring", W, ring, item(kAR, k, n, 0, true), true);
                add_single_and_thrice("rabenseifner", W, rab, item(kAR, k, W == 1 ? n : 2 * n), true);
                add_single_and_thrice("ring", W, ring, item(kRS, k, n), true);
                add_single_and_thrice("ring_gather", W, ring, item(kRED, k, n, 1 % W), true);
            }
            for (OpKind k : {kWide, kScaledHost, kScaledDev}) {
                add_single_and_thrice("wide_staged_ring", W, ring, item(kAR, k, n), true);
                add_single_and_thrice("wide_staged_ring", W, ring, item(kAR, k, n, 0, true), true);
                add_single_and_thrice("wide_staged_rabenseifner", W, rab, item(kAR, k, W == 1 ? n : 2 * n), true);
                add_single_and_thrice("wide_staged_ring", W, ring, item(kRS, k, n), true);
                add_single_and_thrice("wide_staged_ring", W, ring, item(kRED, k, n, 1 % W), true);
            }
            for (OpKind k : {kWidened0, kWidened1}) {
                add_single_and_thrice("wide_staged_ring", W, ring, item(kRS, k, n), true);
                add_single_and_thrice("wide_staged_ring", W, ring, item(kRED, k, n, 1 % W), true);
                if (W > 1) add_single_and_thrice("wide_staged_ring", W, ring, item(kRED, k, n, 0), true);
            }
        }
    // C: pairs of calls on two streams, one pair (at least) per library buffer.
    const size_t n3 = 3 * 1031;
    add_pair("dev_work/reduce_scatter+reduce_scatter", 3, ring, item(kRS, kSum, n3), item(kRS, kSum, n3));
    add_pair("dev_work/reduce+reduce_scatter", 3, ring, item(kRED, kSum, n3, 1), item(kRS, kSum, n3));
    add_pair("dev_work/premul_reduce_scatter+reduce", 3, ring, item(kRS, kPremulDev, n3), item(kRED, kSum, n3, 0));
    add_pair("dev_scratch/all_reduce+all_reduce", 3, ring_pad, item(kAR, kSum, n3), item(kAR, kSum, n3));
    add_pair("dev_scratch/rabenseifner+rabenseifner", 4, rab_pad, item(kAR, kSum, 4 * 1031), item(kAR, kSum, 4 * 1031));
    add_pair("dev_scratch/all_reduce+reduce_scatter", 3, ring_pad, item(kAR, kSum, n3), item(kRS, kSum, n3));
    add_pair("dev_wide/wide_all_reduce+wide_all_reduce", 3, ring, item(kAR, kWide, n3), item(kAR, kWide, n3));
    add_pair("dev_wide/scaled_reduce_scatter+wide_reduce", 3, ring, item(kRS, kScaledDev, n3), item(kRED, kWide, n3, 1));
    add_pair("dev_wide/widened_acc1+widened_acc0", 3, ring, item(kRS, kWidened1, n3), item(kRS, kWidened0, n3));
    add_pair("dev_wide/widened_w1", 1, ring, item(kRS, kWidened1, 1031), item(kRS, kWidened1, 1031));
    add_pair("no_buffer/all_reduce+all_reduce", 3, ring, item(kAR, kSum, n3), item(kAR, kSum, n3));
    add_pair("no_buffer/all_gather+broadcast", 3, ring, item(kAG, kSum, n3), item(kBC, kSum, n3, 1));
    add_pair("no_buffer/w9", 9, direct, item(kAR, kSum, 9 * 8), item(kRS, kSum, 9 * 8));
    // D: groups.
    for (const Env& env : {ring, direct}) {
        const std::string path = env.at("DCCL_ALLREDUCE_ALGORITHM").empty() ? "direct" : "ring";
        const bool ev = path == "ring";
        Scenario sc;
        sc.W = 3;
        sc.env = env;
        sc.event_ordered = ev;
        sc.name = "group/three_streams/" + path;
        sc.phases = {Phase{true, {item(kAR, kSum, 3 * 8, 0, false, 0, 0), item(kAR, kSum, 3 * 1031, 0, false, 1, 1),
                                  item(kAR, kSum, 3 * 257, 0, true, 2, 2)}}};
        g_scenarios.push_back(sc);
        sc.name = "group/two_groups_two_streams/" + path;
        sc.phases = {Phase{true, {item(kRS, kSum, 3 * 8, 0, false, 0, 0), item(kRS, kSum, 3 * 1031, 0, false, 1, 0)}},
                     Phase{true, {item(kRS, kSum, 3 * 8, 0, false, 2, 1), item(kRS, kSum, 3 * 1031, 0, false, 3, 1)}}};
        g_scenarios.push_back(sc);
        sc.name = "group/widened_acc1/" + path;
        sc.phases = {Phase{true, {item(kRS, kWidened1, 3 * 257, 0, false, 0, 0), item(kRS, kWidened1, 3 * 1031, 0, false, 1, 1),
                                  item(kRS, kWidened1, 3 * 3, 0, false, 2, 0)}},
                     Phase{true, {item(kRED, kWidened1, 3 * 257, 1, false, 3, 2), item(kRED, kWidened1, 3 * 8, 1, false, 4, 0)}}};
        g_scenarios.push_back(sc);
        // the mixed queue of tests/test_widened_group.py: [acc0, acc0, acc1, acc1, sum, sum, acc0], bf16 throughout
        // there; the plain sums here are fp32, which keeps them a run of their own just the same
        const size_t counts[] = {257, 1031, 515, 3, 64, 257, 2};
        const OpKind kinds[] = {kWidened0, kWidened0, kWidened1, kWidened1, kSum, kSum, kWidened0};
        for (const char* coalesce : {"", "0"}) {
            Scenario mq;
            mq.W = 4;
            mq.env = env;
            if (*coalesce) mq.env["DCCL_GROUP_COALESCE"] = coalesce;
            mq.event_ordered = ev;
            mq.name = std::string("group/mixed_queue/") + path + (*coalesce ? "/coalesce_off" : "/coalesce_on");
            Phase ph{true, {}};
            for (int i = 0; i < 7; ++i) ph.items.push_back(item(kRS, kinds[i], 4 * counts[i], 0, false, i, i % 2));
            mq.phases = {ph, ph};  // twice, on the same buffers: the second group follows the first with no sync
            g_scenarios.push_back(mq);
        }
    }
}

// --------------------------------------------------------------------------------- hand-written self-check traces
hb::Rec rec(hb::Kind kind, uint64_t stream, uint64_t event, std::vector<hb::Range> ranges = {}) {
    hb::Rec r;
    r.kind = kind, r.stream = stream, r.event = event, r.ranges = std::move(ranges);
    return r;
}
hb::Range rd(uintptr_t lo, uintptr_t hi) { return hb::Range{lo, hi, false}; }
hb::Range wr(uintptr_t lo, uintptr_t hi) { return hb::Range{lo, hi, true}; }

void print_selftest(const char* name, const hb::Trace& t) {
    const hb::Checker chk(t);
    const hb::Report rep = chk.analyse();
    std::string line = std::string("{\"selftest\": \"") + name + "\", \"hazards\": [";
    for (size_t i = 0; i < rep.hazards.size(); ++i)
        line += std::string(i ? ", " : "") + "[" + std::to_string(rep.hazards[i].a) + ", " +
                std::to_string(rep.hazards[i].b) + "]";
    line += "], \"unbound_waits\": [";
    for (size_t i = 0; i < rep.unbound_waits.size(); ++i)
        line += std::string(i ? ", " : "") + std::to_string(rep.unbound_waits[i]);
    line += "], \"cycles\": [";
    for (size_t i = 0; i < rep.cycles.size(); ++i) {
        line += std::string(i ? ", " : "") + "[";
        for (size_t j = 0; j < rep.cycles[i].size(); ++j)
            line += std::string(j ? ", " : "") + std::to_string(rep.cycles[i][j]);
        line += "]";
    }
    line += "], \"load_bearing\": [";
    const std::vector<size_t> lb = hb::load_bearing_waits(chk);
    for (size_t i = 0; i < lb.size(); ++i) line += std::string(i ? ", " : "") + std::to_string(lb[i]);
    line += "]}";
    std::puts(line.c_str());
}

void selftests() {
    using K = hb::Kind;
    constexpr uint64_t A = 1, B = 2, ready = 10, done = 11, e1 = 12, e2 = 13;
    // A ring step: the sender (stream A) fills its chunk and posts it; the receiver (stream B) waits for `ready`,
    // reads the chunk in place, records `done`; the sender waits for `done` (the acknowledgement) and only then lets
    // the user overwrite the chunk.
    const hb::Trace ring_step = {
        rec(K::kOp, A, 0, {wr(0x1000, 0x1100)}),                      // 0 producer
        rec(K::kRecord, A, ready),                                    // 1
        rec(K::kWait, B, ready),                                      // 2
        rec(K::kOp, B, 0, {rd(0x1000, 0x1100), wr(0x2000, 0x2100)}),  // 3 combine from the peer's chunk
        rec(K::kRecord, B, done),                                     // 4
        rec(K::kWait, A, done),                                       // 5 the acknowledgement
        rec(K::kOp, A, 0, {wr(0x1000, 0x1100)}),                      // 6 clobber
    };
    print_selftest("ring_step", ring_step);
    hb::Trace no_ack = ring_step;
    no_ack.erase(no_ack.begin() + 5);
    print_selftest("ring_step_without_ack", no_ack);
    // Library scratch written by two calls on two streams: without an event the second call's staging copy and
    // the first call's copy out of the scratch are unordered.
    const hb::Trace scratch = {
        rec(K::kOp, A, 0, {rd(0x1000, 0x1100), wr(0x9000, 0x9100)}),  // 0 call 1 stages into the scratch
        rec(K::kOp, A, 0, {rd(0x9000, 0x9100), wr(0x2000, 0x2100)}),  // 1 call 1 copies its result out
        rec(K::kRecord, A, e1),                                       // 2
        rec(K::kWait, B, e1),                                         // 3
        rec(K::kOp, B, 0, {rd(0x3000, 0x3100), wr(0x9000, 0x9100)}),  // 4 call 2 stages into the scratch
    };
    print_selftest("scratch_two_streams", scratch);
    hb::Trace no_event = {scratch[0], scratch[1], scratch[4]};
    print_selftest("scratch_two_streams_without_event", no_event);
    // A wait that precedes its record in host order is a no-op under HIP's rule: the hazard stays, the wait is
    // reported as unbound.
    const hb::Trace early_wait = {
        rec(K::kWait, B, e1),                     // 0
        rec(K::kOp, A, 0, {wr(0x1000, 0x1100)}),  // 1
        rec(K::kRecord, A, e1),                   // 2
        rec(K::kOp, B, 0, {rd(0x1000, 0x1100)}),  // 3
    };
    print_selftest("wait_before_record", early_wait);
    // Two streams that each wait for the other's NEXT record: nothing under HIP's rule (both waits are no-ops), a
    // deadlock for a runtime that binds late.
    const hb::Trace cycle = {
        rec(K::kWait, A, e2),    // 0
        rec(K::kRecord, A, e1),  // 1
        rec(K::kWait, B, e1),    // 2
        rec(K::kRecord, B, e2),  // 3
    };
    print_selftest("late_binding_cycle", cycle);
    // A host synchronisation orders what it covers before everything issued later, by any stream.
    const hb::Trace synced = {
        rec(K::kOp, A, 0, {wr(0x1000, 0x1100)}),  // 0
        rec(K::kSync, A, 0),                      // 1 hipStreamSynchronize(A)
        rec(K::kOp, B, 0, {rd(0x1000, 0x1100)}),  // 2
        rec(K::kOp, A, 0, {wr(0x1000, 0x1100)}),  // 3 not covered by the sync: unordered with 2
    };
    print_selftest("host_sync", synced);
}

}  // namespace

int main(int argc, char** argv) {
    const auto t0 = std::chrono::steady_clock::now();
    const char* only = argc > 1 ? argv[1] : nullptr;  // run the scenarios whose name contains this
    selftests();
    build_scenarios();
    size_t ran = 0;
    for (const Scenario& sc : g_scenarios) {
        if (only != nullptr && sc.name.find(only) == std::string::npos) continue;
        run_scenario(sc);
        ++ran;
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"summary\": true, \"scenarios\": %zu, \"failed\": %d, \"seconds\": %.2f}\n", ran, g_failed_scenarios, s);
    return 0;
}
