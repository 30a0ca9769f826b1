// lbm_order.hpp -- the ordering of the two streams of a context: the state that is carried from one launch unit to the next (class
// Order, the only reader and writer of it) and the skeletons of a two-stream and of a one-stream unit, which issue every event
// operation between the streams.  Plain C++, nothing from HIP: the device is a parameter `Dev` with
//     int record(Event, Stream);   int wait(Stream, Event);      (LBM_OK or an error code; the first error is passed through)
// which the library maps onto the context's streams and events (HipDev, lbm_host.hpp) and tests/test_order_cpu.py replaces by one
// that prints -- its only purpose: that test drives exactly this code through every short sequence of units and checks the
// happens-before relation of what was enqueued.
//
// Every launch unit (a single step or S steps in one launch) of a slab, and a unit of a lone lattice whose wall frame runs beside the
// bulk kernel, uses both streams.  Unit n goes lat[a] -> lat[b]; E = its halo exchange, G = its edge work (the slab's edge rows / the
// frame passes / the edge launch of the streaming kernel), B = its bulk kernel:
//     COMM (highest priority):  [E_n]  wait(INT: B_{n-1})  [record GO]  G_n  record EDGES
//     COMPUTE:                  wait(EDGES: G_{n-1})  [wait GO]  B_n  record INT
// (an event is re-recorded every unit: a wait refers to the last record before it in host order -- the one named above).  Why this
// orders everything that must be ordered, F being the rows G writes next to each interface (the frame width; 1 for a single step):
//   * E_n sends the `rows` rows of lat[a] next to each interface and fills lat[a]'s ghost rows.  It is enqueued FIRST, ahead of the
//     wait for B_{n-1}, so that it runs beside that kernel.  That is right when the rows it sends were written on COMM itself, by
//     G_{n-1}: edge_rows >= rows.  After a single step only one row was (a deep exchange of S rows follows one at the second unit of
//     every run and after a tail), and at the start of a call, or after one-stream work, none: the lattice may come from an upload, an
//     import, a recomputation or a lone unit on COMPUTE.  Then before_exchange() makes COMM wait for INT first.  (r01 missed this;
//     only a soak of several solvers in one process found the race.)  Nothing else touches those rows or lat[a]'s ghost rows
//     meanwhile: B_{n-1}, which may still run, writes lat[a]'s rows [F, ny - F) only and reads lat[b].
//   * G_n reads lat[a] up to F + S - 1 rows from an interface plus the ghost rows: written by G_{n-1} and E_n (same stream, earlier)
//     and by B_{n-1} (the wait on INT sits between E_n and G_n).  It writes lat[b]'s edge rows, last read by G_{n-1} / E_{n-1} (same
//     stream, earlier) and by B_{n-1} (waited for).
//   * B_n reads lat[a]'s rows from F - (S - 1) on: B_{n-1}'s (same stream) and G_{n-1}'s (the wait on EDGES, recorded after G_{n-1}).
//     It writes lat[b]'s rows [F, ny - F): last read by B_{n-1} (same stream) and G_{n-1} (waited for).  The next exchange E_{n+1},
//     which may run beside B_n, touches lat[b]'s edge and ghost rows only -- disjoint from B_n's.
//   * GO (hold_bulk) only ADDS an edge: B_n after everything COMM had enqueued when it was recorded (E_n and the wait for B_{n-1}).
//     It is recorded (host order) before COMPUTE is told to wait for it, and what it waits for -- INT of unit n - 1 -- was recorded on
//     COMPUTE before that wait: no cycle, no wait on an event not yet recorded.  Its price: B_n also waits for E_n, which it does not
//     need; E_n has had the whole of B_{n-1} to finish, so this costs only when a neighbour is that late -- and then G_n, which
//     B_{n+1} needs, waits for the same exchange anyway.
//   * One-stream work on COMPUTE (a lone unit in one launch, an automatic sample, the replay of the lagged lattice) neither records INT
//     nor waits for EDGES unless G of an earlier unit is still unwaited-for -- two event operations per unit are 7 - 8 % of a
//     launch-bound lattice's step (160^2: 3.51 -> 3.24 us).  Instead it leaves INT stale, and whoever next makes COMM wait for INT
//     records it first; and it sets edge_rows = 0, so the next exchange waits for it whichever context it runs in.
//   * A call ends with end_call(): COMPUTE waits for everything on COMM (exports, timing events, externally driven calls use COMPUTE
//     alone), and the next call begins by recording INT behind whatever they enqueued.
#pragma once

#include "../../include/lbm.h"

namespace lbmhost {

enum class Event { INT, EDGES, GO, HALO };
enum class Stream { COMPUTE, COMM };

class Order {
  public:
    // both streams have been synchronised and the lattice is replaced (init, upload)
    void reset() { int_stale_ = edges_pending_ = thin_valid_ = false; edge_rows_ = 0; }

    // The one-row halo of lat[cur] is in place: exchanged on COMM by the call that ended last, for the field export; the next
    // unit skips its one-row exchange.
    bool thin_valid() const { return thin_valid_; }
    void set_thin_valid(bool v) { thin_valid_ = v; }

    // Start of a stepping call.  two_streams: the context ever uses COMM (a lone lattice stepping one step per launch does not, and
    // records nothing).  INT then covers everything enqueued so far: init, upload, imported rows, earlier calls.
    template <class Dev>
    int begin_call(Dev& d, bool two_streams) {
        edge_rows_ = 0;   // the first exchange of the call waits for INT
        if (!two_streams) return LBM_OK;
        int_stale_ = false;
        return d.record(Event::INT, Stream::COMPUTE);
    }

    // Before an exchange that sends `rows` rows per interface is enqueued on COMM.
    template <class Dev>
    int before_exchange(Dev& d, int rows) {
#ifdef LBM_DEBUG
        if (debug_no_exchange_ready) return LBM_OK;
#endif
        return edge_rows_ < rows ? comm_waits_int(d) : LBM_OK;
    }

    // A two-stream unit opens: G may follow on COMM, B on COMPUTE.
    template <class Dev>
    int open_unit(Dev& d) {
        const int rc = comm_waits_int(d);
        return rc ? rc : d.wait(Stream::COMPUTE, Event::EDGES);
    }

    // B becomes ready one cross-stream hop behind G (where B would otherwise take every CU first: see run_unit).
    template <class Dev>
    int hold_bulk(Dev& d) {
        const int rc = d.record(Event::GO, Stream::COMM);
        return rc ? rc : d.wait(Stream::COMPUTE, Event::GO);
    }

    // G has been enqueued on COMM; it writes `rows` rows next to each interface.
    template <class Dev>
    int edges_done(Dev& d, int rows) {
        edges_pending_ = true;
        edge_rows_ = rows;
        return d.record(Event::EDGES, Stream::COMM);
    }

    // B has been enqueued on COMPUTE.
    template <class Dev>
    int bulk_done(Dev& d) {
        int_stale_ = false;
        return d.record(Event::INT, Stream::COMPUTE);
    }

    // Work that reads or writes the lattice is about to be enqueued on COMPUTE alone.
    template <class Dev>
    int one_stream(Dev& d) {
        int_stale_ = true;
        edge_rows_ = 0;
        if (!edges_pending_) return LBM_OK;
        edges_pending_ = false;
        return d.wait(Stream::COMPUTE, Event::EDGES);
    }

    // End of a call that used COMM: later work on COMPUTE alone sees what COMM wrote.
    template <class Dev>
    int end_call(Dev& d) {
        const int rc = d.record(Event::HALO, Stream::COMM);
        return rc ? rc : d.wait(Stream::COMPUTE, Event::HALO);
    }

#ifdef LBM_DEBUG
    bool debug_no_exchange_ready = false;   // before_exchange() never waits: shows that the tests see the race (LBM_DEBUG_NO_EXCHANGE_READY)
#endif

  private:
    template <class Dev>
    int comm_waits_int(Dev& d) {
        if (int_stale_) {
            int_stale_ = false;
            const int rc = d.record(Event::INT, Stream::COMPUTE);
            if (rc) return rc;
        }
        return d.wait(Stream::COMM, Event::INT);
    }

    bool int_stale_ = false;      // COMPUTE has work that INT does not cover yet
    bool edges_pending_ = false;  // EDGES was recorded and COMPUTE has not been made to wait for it since
    bool thin_valid_ = false;
    int edge_rows_ = 0;           // rows next to each interface of lat[cur] that work on COMM wrote, and COMM's stream order therefore covers
};

// A two-stream unit.  exchange_rows: rows per interface that `exchange` sends (0: the unit has none, `exchange` is not called);
// hold: release the bulk work behind the edge work; edge_rows: rows per interface that `edge` writes.  The three callables enqueue
// their work -- exchange and edge on COMM, bulk on COMPUTE -- and return LBM_OK or an error code.
template <class Dev, class X, class G, class B>
int two_stream_unit(Order& o, Dev& d, int exchange_rows, bool hold, int edge_rows, X&& exchange, G&& edge, B&& bulk) {
    int rc = LBM_OK;
    if (exchange_rows > 0) {
        rc = o.before_exchange(d, exchange_rows);
        if (rc == LBM_OK) rc = exchange();
    }
    if (rc == LBM_OK) rc = o.open_unit(d);
    if (rc == LBM_OK && hold) rc = o.hold_bulk(d);
    if (rc == LBM_OK) rc = edge();
    if (rc == LBM_OK) rc = o.edges_done(d, edge_rows);
    if (rc == LBM_OK) rc = bulk();
    if (rc == LBM_OK) rc = o.bulk_done(d);
    return rc;
}

// A one-stream unit: `work` enqueues on COMPUTE alone.
template <class Dev, class W>
int one_stream_unit(Order& o, Dev& d, W&& work) {
    const int rc = o.one_stream(d);
    return rc ? rc : work();
}
}  // namespace lbmhost
