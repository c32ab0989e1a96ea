// con_parse_fuzz.cpp -- a stand-alone run of the handshake's host-only parsers (jeromq_amd/csrc/
// cz_hs_parse.cpp: command dispatch, WELCOME / READY framing, the ERROR parse, the metadata block)
// over a seeded stream of truncated, oversized and bit-flipped WELCOME, READY and ERROR commands.
// Built for the CPU with the address and undefined-behaviour sanitizers (tests/test_connector_host.py):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include
//       tools/con_parse_fuzz.cpp jeromq_amd/csrc/cz_hs_parse.cpp -o con_parse_fuzz
// Every command lives in a heap block of exactly its size, so a read past its end is a report.  It
// opens no device.  Usage: con_parse_fuzz [iterations per parser, default 100000] [seed].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../include/curvezmq_mi355x.h"
#include "../jeromq_amd/csrc/cz_hs_parse.h"

using namespace czi;

namespace {

uint64_t g_state;

uint64_t rnd()  // splitmix64
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

std::vector<uint8_t> random_bytes(size_t n)
{
    std::vector<uint8_t> v(n);
    for (auto &b : v)
        b = (uint8_t)rnd();
    return v;
}

std::vector<uint8_t> concat(const char *head, size_t head_len, const std::vector<uint8_t> &tail)
{
    std::vector<uint8_t> v(head, head + head_len);
    v.insert(v.end(), tail.begin(), tail.end());
    return v;
}

std::vector<uint8_t> a_property(const char *name, const std::vector<uint8_t> &value)
{
    std::vector<uint8_t> v;
    v.push_back((uint8_t)strlen(name));
    v.insert(v.end(), name, name + strlen(name));
    for (int s = 24; s >= 0; s -= 8)
        v.push_back((uint8_t)(value.size() >> s));
    v.insert(v.end(), value.begin(), value.end());
    return v;
}

std::vector<uint8_t> a_metadata()
{
    static const char *types[] = {"PAIR", "ROUTER", "DEALER", "PUB", "SUB", "NOPE", ""};
    const char *t = types[rnd() % 7];
    std::vector<uint8_t> m = a_property("Socket-Type", std::vector<uint8_t>(t, t + strlen(t)));
    if (rnd() & 1) {
        const std::vector<uint8_t> id = a_property("Identity", random_bytes(rnd() % 222));
        m.insert(m.end(), id.begin(), id.end());
    }
    return m;
}

// a well-formed command of one of the three kinds (kind 3: the metadata block alone)
std::vector<uint8_t> well_formed(int kind)
{
    switch (kind) {
    case 0:
        return concat("\x07WELCOME", 8, random_bytes(160));
    case 1:
        return concat("\x05READY", 6, random_bytes(8 + 16 + 1 + rnd() % 256));
    case 2: {
        static const char *reasons[] = {"", "300", "400", "500", "abc", "40", "4000", "200"};
        const char *r = reasons[rnd() % 8];
        std::vector<uint8_t> v = concat("\x05" "ERROR", 6, {});
        if (rnd() % 8) {
            v.push_back((uint8_t)strlen(r));
            v.insert(v.end(), r, r + strlen(r));
        }
        return v;
    }
    default:
        return a_metadata();
    }
}

// truncate, extend, flip bits, overwrite a length field: what a hostile or broken peer sends
void mutate(std::vector<uint8_t> &v)
{
    switch (rnd() % 6) {
    case 0:
        break;
    case 1:
        v.resize(rnd() % (v.size() + 1));
        break;
    case 2: {
        const std::vector<uint8_t> more = random_bytes(1 + rnd() % 600);
        v.insert(v.end(), more.begin(), more.end());
        break;
    }
    case 3:
        for (int k = 1 + (int)(rnd() % 4); k > 0 && !v.empty(); k--)
            v[rnd() % v.size()] ^= (uint8_t)(1u << (rnd() % 8));
        break;
    case 4:
        if (!v.empty())
            v[rnd() % (v.size() < 24 ? v.size() : 24)] = (uint8_t)rnd();
        break;
    default:
        v.resize(rnd() % (v.size() + 1));
        for (int k = (int)(rnd() % 3); k > 0 && !v.empty(); k--)
            v[rnd() % v.size()] ^= (uint8_t)(1u << (rnd() % 8));
        break;
    }
}

// the bytes in a block of exactly their size (size 0: a one-byte block nobody may read)
struct Exact {
    std::unique_ptr<uint8_t[]> p;
    uint64_t size;
    explicit Exact(const std::vector<uint8_t> &v) : p(new uint8_t[v.empty() ? 1 : v.size()]), size(v.size())
    {
        if (!v.empty())
            memcpy(p.get(), v.data(), v.size());
    }
};

int check(bool ok, const char *what)
{
    if (!ok)
        fprintf(stderr, "con_parse_fuzz: %s\n", what);
    return ok ? 0 : 1;
}

// what the parsers must say about commands whose answer is known
int known_answers()
{
    int bad = 0;
    const std::vector<uint8_t> w = concat("\x07WELCOME", 8, std::vector<uint8_t>(160));
    bad += check(client_command(w.data(), w.size()) == CLIENT_CMD_WELCOME && welcome_framing(168) == 0, "WELCOME");
    bad += check(welcome_framing(167) == CZ_ZMTP_MALFORMED_COMMAND_READY && welcome_framing(169) != 0, "WELCOME sizes");
    const std::vector<uint8_t> r = concat("\x05READY", 6, std::vector<uint8_t>(24));
    bad += check(client_command(r.data(), r.size()) == CLIENT_CMD_READY && ready_framing(30) == 0, "READY");
    bad += check(ready_framing(29) == CZ_ZMTP_MALFORMED_COMMAND_READY && ready_framing(286) == 0 &&
                     ready_framing(287) == CZ_ZMTP_MALFORMED_COMMAND_READY, "READY sizes");
    bad += check(client_command(r.data(), 5) == CLIENT_CMD_UNKNOWN && client_command(r.data(), 0) == CLIENT_CMD_UNKNOWN,
                 "short command");
    int st = 0, ev = 0;
    bad += check(parse_error_command((const uint8_t *)"\x05" "ERROR\x03" "400", 10, &st, &ev) == CZ_OK && st == 400 &&
                     ev == 0, "ERROR 400");
    st = ev = 0;
    bad += check(parse_error_command((const uint8_t *)"\x05" "ERROR\x03" "abc", 10, &st, &ev) == CZ_EPROTO && st == 0 &&
                     ev == CZ_ZAP_MALFORMED_REPLY, "ERROR abc");
    st = ev = 0;
    bad += check(parse_error_command((const uint8_t *)"\x05" "ERROR\x09" "ab", 9, &st, &ev) == CZ_EPROTO &&
                     ev == CZ_ZMTP_MALFORMED_COMMAND_ERROR, "ERROR overrun");
    st = ev = 0;
    bad += check(parse_error_command((const uint8_t *)"\x05" "ERROR\x00", 7, &st, &ev) == CZ_OK && st == 0 && ev == 0,
                 "ERROR empty");
    const std::vector<uint8_t> m = a_property("Socket-Type", {'R', 'O', 'U', 'T', 'E', 'R'});
    Props props;
    bad += check(parse_metadata(m.data(), m.size(), 5, &props) == CZ_OK && props.size() == 1, "metadata DEALER-ROUTER");
    bad += check(parse_metadata(m.data(), m.size(), 1, nullptr) == CZ_EINVAL, "metadata PUB-ROUTER");
    bad += check(parse_metadata(m.data(), m.size() - 1, 5, nullptr) == CZ_EPROTO, "metadata truncated");
    return bad;
}

}  // namespace

int main(int argc, char **argv)
{
    const long iters = argc > 1 ? atol(argv[1]) : 100000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 0x6a65726f6d71ull;
    int bad = known_answers();
    uint64_t sink = 0;
    long counts[4] = {0, 0, 0, 0};
    // 1. dispatch + framing, as cz_hs and the connector run them: every kind of command
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> v = well_formed((int)(rnd() % 3));
        mutate(v);
        const Exact e(v);
        const ClientCommand c = client_command(e.p.get(), e.size);
        sink += (uint64_t)c + (uint64_t)welcome_framing(e.size) + (uint64_t)ready_framing(e.size);
        bad += check(c == CLIENT_CMD_UNKNOWN || e.size >= 6, "a command named with fewer than 6 bytes");
        if (c == CLIENT_CMD_READY && ready_framing(e.size) == 0)
            bad += check(e.size >= 30 && e.size - 30 <= 256, "READY framing let a size through");
        counts[0]++;
    }
    // 2. the ERROR parse, on whatever the dispatch takes for an ERROR (and on everything else named so)
    for (long it = 0; it < iters; it++) {
        std::vector<uint8_t> v = well_formed(2);
        mutate(v);
        const Exact f(v);
        int st = 0, ev = 0;
        const int rc = parse_error_command(f.p.get(), f.size, &st, &ev);
        bad += check(rc == CZ_OK ? ev == 0 && (st == 0 || st == 300 || st == 400 || st == 500) : rc == CZ_EPROTO && ev != 0,
                     "ERROR parse result");
        sink += (uint64_t)rc + (uint64_t)st;
        counts[1]++;
    }
    // 3. the metadata parser on mutated metadata blocks, and 4. on the tail of mutated READY plaintexts
    for (int pass = 0; pass < 2; pass++)
        for (long it = 0; it < iters; it++) {
            std::vector<uint8_t> v = pass == 0 ? a_metadata() : random_bytes(rnd() % 257);
            if (pass == 1 && !v.empty() && (rnd() & 1)) {
                const std::vector<uint8_t> m = a_metadata();
                memcpy(v.data(), m.data(), m.size() < v.size() ? m.size() : v.size());
            }
            mutate(v);
            const Exact e(v);
            Props props;
            const int rc = parse_metadata(e.p.get(), e.size, (int)(rnd() % 21), (rnd() & 1) ? &props : nullptr);
            bad += check(rc == CZ_OK || rc == CZ_EPROTO || rc == CZ_EINVAL, "metadata parse result");
            uint64_t total = 0;
            for (const auto &p : props)
                total += p.first.size() + p.second.size();
            bad += check(total <= e.size, "metadata properties larger than the block");
            sink += (uint64_t)rc + total;
            counts[2 + pass]++;
        }
    printf("con_parse_fuzz: dispatch %ld, error %ld, metadata %ld + %ld, %d failed checks (sink %llx)\n", counts[0],
           counts[1], counts[2], counts[3], bad, (unsigned long long)sink);
    return bad ? 1 : 0;
}
