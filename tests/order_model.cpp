// order_model.cpp -- the library's two-stream ordering (csrc/lbm_order.hpp: class Order and the skeletons of a unit) on a device
// that prints, for tests/test_order_cpu.py.  It drives the real code through every sequence of up to `maxlen` items of an alphabet,
// depth first, so that a sequence's trace is the lines from the root to its node:
//   alphabet NAME / push ITEM kind S exchange_rows hold rows_of_the_edge_work / rec EVENT STREAM / wait STREAM EVENT / work STREAM LABEL /
//   endcall / pop
// kind: two (a two-stream unit), one (a one-stream unit), sample (an automatic sample), call (a call boundary: what step_many does
// at the end of a call and at the start of the next, S = 1 with foreign work on COMPUTE in between).  LABEL: E exchange, G edge
// work, B bulk work, W one-stream work, F foreign work.
// usage: order_model ALPHABET MAXLEN [noready]      (noready: a build with -DLBM_DEBUG, Order::debug_no_exchange_ready set)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lbm_order.hpp"

using namespace lbmhost;

static const char* name(Event e) { return e == Event::INT ? "INT" : e == Event::EDGES ? "EDGES" : e == Event::GO ? "GO" : "HALO"; }
static const char* name(Stream s) { return s == Stream::COMPUTE ? "COMPUTE" : "COMM"; }

struct PrintDev {
    int record(Event e, Stream s) { std::printf("rec %s %s\n", name(e), name(s)); return LBM_OK; }
    int wait(Stream s, Event e) { std::printf("wait %s %s\n", name(s), name(e)); return LBM_OK; }
    int work(Stream s, const char* label) { std::printf("work %s %s\n", name(s), label); return LBM_OK; }
};

constexpr int F = 12;   // the frame width of the modelled context: what the edge work of a multi-step unit covers (a single step: 1)

struct Item {
    const char* id;
    const char* kind;
    int S, exchange_rows, hold;   // (call: S = 1 marks foreign work between the calls)
};
static const Item SLAB[] = {{"call_foreign", "call", 1, 0, 0}, {"s1_x1", "two", 1, 1, 0}, {"s1", "two", 1, 0, 0},   {"s8_x8_hold", "two", 8, 8, 1},
                            {"s8_x8", "two", 8, 8, 0},         {"s8", "two", 8, 0, 0},    {"s4_x1", "two", 4, 1, 0}, {"s4_x4", "two", 4, 4, 0}};
static const Item LONE[] = {{"call", "call", 0, 0, 0}, {"one", "one", 8, 0, 0}, {"sample", "sample", 0, 0, 0}, {"beside8", "two", 8, 0, 0}, {"beside4", "two", 4, 0, 0}};

// the run state of the modelled context beside its Order: what step_many keeps per call
struct Run {
    Order order;
    bool comm_used = false;
};

static int run_item(Run& r, PrintDev& d, const Item& it) {
    const int covers = it.S > 1 ? F : 1;   // rows next to each interface that the edge work writes
    std::printf("push %s %s %d %d %d %d\n", it.id, it.kind, it.S, it.exchange_rows, it.hold, !std::strcmp(it.kind, "two") ? covers : 0);
    if (!std::strcmp(it.kind, "two")) {
        r.comm_used = true;
        return two_stream_unit(
            r.order, d, it.exchange_rows, it.hold != 0, covers, [&] { return d.work(Stream::COMM, "E"); }, [&] { return d.work(Stream::COMM, "G"); },
            [&] { return d.work(Stream::COMPUTE, "B"); });
    }
    if (!std::strcmp(it.kind, "one")) return one_stream_unit(r.order, d, [&] { return d.work(Stream::COMPUTE, "W"); });
    if (!std::strcmp(it.kind, "sample")) {   // (sample_if_due)
        const int rc = r.order.one_stream(d);
        return rc ? rc : d.work(Stream::COMPUTE, "W");
    }
    // the end of a call and the start of the next (step_many)
    int rc = LBM_OK;
    if (r.comm_used) {
        rc = r.order.end_call(d);
        std::printf("endcall\n");
    }
    r.comm_used = false;
    if (rc == LBM_OK && it.S) rc = d.work(Stream::COMPUTE, "F");
    if (rc == LBM_OK) rc = r.order.begin_call(d, true);
    return rc;
}

static int walk(const Run& r, const std::vector<Item>& alphabet, int left) {
    if (left == 0) return LBM_OK;
    for (const Item& it : alphabet) {
        Run next = r;
        PrintDev d;
        int rc = run_item(next, d, it);
        if (rc == LBM_OK) rc = walk(next, alphabet, left - 1);
        if (rc) return rc;
        std::printf("pop\n");
    }
    return LBM_OK;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::vector<Item> alphabet;
    if (std::strcmp(argv[1], "lone")) alphabet.insert(alphabet.end(), std::begin(SLAB), std::end(SLAB));
    if (std::strcmp(argv[1], "slab")) alphabet.insert(alphabet.end(), std::begin(LONE), std::end(LONE));
    Run r;
    if (argc > 3) {
#ifdef LBM_DEBUG
        r.order.debug_no_exchange_ready = true;
#else
        return 2;
#endif
    }
    std::printf("alphabet %s\n", argv[1]);
    PrintDev d;
    int rc = r.order.begin_call(d, true);   // every sequence starts inside a call
    if (rc == LBM_OK) rc = walk(r, alphabet, std::atoi(argv[2]));
    return rc;
}
