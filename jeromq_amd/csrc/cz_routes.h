// cz_routes.h -- the engine's forward routes (cz_engine_forward): which connection's received bytes leave
// re-sealed for which other connection.  Plain host C++ with no device call, so the rules can be run without
// an engine (tests/test_relay_streams_host.py compiles this header into a stand-alone program).
//
// ONE SOURCE PER DESTINATION: the relay re-seals a source's stream in place into the destination's outbound
// stream, so a destination takes the bytes of one source.  Several sources sharing a destination need the
// whole-message cut (cz_relay_stream_result::whole_bytes) and an out-of-place pass: open.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace czi {

struct RouteTable {
    std::vector<int32_t> to;    // to[from]: the destination, -1 none
    std::vector<int32_t> from;  // from[to]: the source, -1 none

    int dest(int f) const { return f >= 0 && (size_t)f < to.size() ? to[(size_t)f] : -1; }
    int source(int t) const { return t >= 0 && (size_t)t < from.size() ? from[(size_t)t] : -1; }

    // Route f -> t (t == -1: clear f's route).  live(id): the id names a connection that has not been removed.
    // false: an unknown or removed id, f == t, or a t that another live route already names (nothing changes).
    template <class Live>
    bool set(int f, int t, Live live)
    {
        if (!live(f) || (t != -1 && (!live(t) || t == f)))
            return false;
        if (t != -1 && source(t) != -1 && source(t) != f)
            return false;
        const size_t need = (size_t)(f > t ? f : t) + 1;
        if (to.size() < need) {
            to.resize(need, -1);
            from.resize(need, -1);
        }
        if (to[(size_t)f] != -1)
            from[(size_t)to[(size_t)f]] = -1;
        to[(size_t)f] = t;
        if (t != -1)
            from[(size_t)t] = f;
        return true;
    }

    // the connection is gone: the route it is the source of and the route it is the destination of
    void drop(int id)
    {
        if (id < 0 || (size_t)id >= to.size())
            return;
        if (to[(size_t)id] != -1)
            from[(size_t)to[(size_t)id]] = -1;
        if (from[(size_t)id] != -1)
            to[(size_t)from[(size_t)id]] = -1;
        to[(size_t)id] = from[(size_t)id] = -1;
    }
};

}  // namespace czi
