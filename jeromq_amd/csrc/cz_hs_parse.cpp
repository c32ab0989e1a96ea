// cz_hs_parse.cpp -- host-only parsers of the CURVE handshake (cz_hs_parse.h): no HIP, no device.
//
// Mirrors Msgs.startsWith (zmq/io/Msgs.java:20-39), Sockets.compatible (zmq/socket/Sockets.java:241-244),
// Mechanism.addProperty :101-116, parseMetadata :140-165, parseErrorMessage :218-241,
// handleErrorReason :243-263, Metadata.read (zmq/io/Metadata.java:365-417) and the command dispatch
// and size checks of CurveClientMechanism.processHandshakeCommand :105-124, processWelcome :281-288
// and processReady :387-395.
#include "cz_hs_parse.h"

#include <cstring>

#include "../../include/curvezmq_mi355x.h"

namespace czi {

// zmq/socket/Sockets.java: names by ZMQ_* type (the enum ordinal) and their compatible peers
namespace {
struct SockType {
    const char *name;
    const char *peers[3];
};
const SockType SOCK_TYPES[] = {
    {"PAIR", {"PAIR"}},          {"PUB", {"SUB", "XSUB"}},       {"SUB", {"PUB", "XPUB"}},
    {"REQ", {"REP", "ROUTER"}},  {"REP", {"REQ", "DEALER"}},     {"DEALER", {"REP", "DEALER", "ROUTER"}},
    {"ROUTER", {"REQ", "DEALER", "ROUTER"}}, {"PULL", {"PUSH"}}, {"PUSH", {"PULL"}},
    {"XPUB", {"SUB", "XSUB"}},   {"XSUB", {"PUB", "XPUB"}},      {"STREAM", {}},
    {"SERVER", {"CLIENT"}},      {"CLIENT", {"SERVER"}},         {"RADIO", {"DISH"}},
    {"DISH", {"RADIO"}},         {"CHANNEL", {"CHANNEL"}},       {"PEER", {"PEER"}},
    {"RAW", {}},                 {"SCATTER", {"GATHER"}},        {"GATHER", {"SCATTER"}},
};
constexpr int NSOCK = (int)(sizeof(SOCK_TYPES) / sizeof(SOCK_TYPES[0]));
constexpr int ZMQ_REQ = 3, ZMQ_DEALER = 5, ZMQ_ROUTER = 6;
}  // namespace

int sock_types() { return NSOCK; }

bool compatible(int self, const std::string &peer)
{
    if (self < 0 || self >= NSOCK)
        return false;
    for (const char *p : SOCK_TYPES[self].peers)
        if (p && peer == p)
            return true;
    return false;
}

// Msgs.startsWith(msg, data, true): the length byte, then bytes 1..len-1 against data[0..len-2]
// (the loop never reaches the last character: the reference's quirk, mirrored)
bool starts_with(const uint8_t *m, uint64_t size, const char *data)
{
    const uint64_t len = strlen(data);
    if (size < len + 1 || m[0] != len)
        return false;
    for (uint64_t i = 1; i < len; i++)
        if (m[i] != (uint8_t)data[i - 1])
            return false;
    return true;
}

uint64_t get_be64(const uint8_t *p)
{
    uint64_t v = 0;
    for (int i = 0; i < 8; i++)
        v = (v << 8) | p[i];
    return v;
}

void put_be64(uint8_t *p, uint64_t v)
{
    for (int i = 7; i >= 0; i--, v >>= 8)
        p[i] = (uint8_t)v;
}

// Mechanism.addProperty: name length byte, name, BE32 value length, value
static void add_property(std::vector<uint8_t> &b, const char *name, const uint8_t *value, uint32_t vlen)
{
    const size_t n = strlen(name);
    b.push_back((uint8_t)n);
    b.insert(b.end(), name, name + n);
    for (int s = 24; s >= 0; s -= 8)
        b.push_back((uint8_t)(vlen >> s));
    if (vlen)
        b.insert(b.end(), value, value + vlen);
}

// Metadata.read + Mechanism.parseMetadata's listener: CZ_OK, CZ_EPROTO (trailing bytes that are not
// a whole property) or CZ_EINVAL (a Socket-Type the local type is not compatible with)
int parse_metadata(const uint8_t *buf, uint64_t len, int self_type, Props *out)
{
    uint64_t left = len, i = 0;
    while (left > 1) {
        const uint32_t nl = buf[i];
        if (nl == 0)
            break;
        i++;
        left--;
        if (left < nl)
            break;
        std::string name((const char *)buf + i, nl);
        i += nl;
        left -= nl;
        if (left < 4)
            break;
        const int32_t vl = (int32_t)(((uint32_t)buf[i] << 24) | ((uint32_t)buf[i + 1] << 16) |
                                     ((uint32_t)buf[i + 2] << 8) | buf[i + 3]);
        i += 4;
        left -= 4;
        if (vl < 0 || left < (uint64_t)vl)
            break;
        std::string value((const char *)buf + i, (size_t)vl);
        if (name == "Socket-Type" && !compatible(self_type, value))
            return CZ_EINVAL;
        if (out)
            out->push_back({name, std::vector<uint8_t>(buf + i, buf + i + vl)});
        i += (uint64_t)vl;
        left -= (uint64_t)vl;
    }
    return left > 0 ? CZ_EPROTO : CZ_OK;
}

// the metadata block a socket of this type sends in INITIATE / READY: Socket-Type and, for REQ / DEALER /
// ROUTER, Identity
std::vector<uint8_t> zmtp_metadata(int socket_type, const uint8_t *identity, size_t identity_len)
{
    std::vector<uint8_t> b;
    const char *tn = socket_type >= 0 && socket_type < NSOCK ? SOCK_TYPES[socket_type].name : "";
    add_property(b, "Socket-Type", (const uint8_t *)tn, (uint32_t)strlen(tn));
    if (socket_type == ZMQ_REQ || socket_type == ZMQ_DEALER || socket_type == ZMQ_ROUTER)
        add_property(b, "Identity", identity, (uint32_t)identity_len);
    return b;
}

ClientCommand client_command(const uint8_t *m, uint64_t size)
{
    if (size >= 8 && starts_with(m, size, "WELCOME"))
        return CLIENT_CMD_WELCOME;
    if (size >= 6 && starts_with(m, size, "READY"))
        return CLIENT_CMD_READY;
    if (size >= 6 && starts_with(m, size, "ERROR"))
        return CLIENT_CMD_ERROR;
    return CLIENT_CMD_UNKNOWN;
}

int welcome_framing(uint64_t size)
{
    return size != 168 ? CZ_ZMTP_MALFORMED_COMMAND_READY : 0;  // sic: the reference's event for a bad WELCOME
}

int ready_framing(uint64_t size)
{
    if (size < 30)
        return CZ_ZMTP_MALFORMED_COMMAND_READY;
    if (16 + size - 14 > 16 + 16 + 256)  // the reference's readyBox capacity (it would throw)
        return CZ_ZMTP_MALFORMED_COMMAND_READY;
    return 0;
}

int parse_error_command(const uint8_t *m, uint64_t size, int *auth_status, int *event)
{
    // Mechanism.parseErrorMessage
    if (size < 7 && size != 6) {
        *event = CZ_ZMTP_MALFORMED_COMMAND_ERROR;
        return CZ_EPROTO;
    }
    if (size >= 7) {
        const int8_t reason_len = (int8_t)m[6];  // a Java byte
        if (reason_len > (int64_t)size - 7) {
            *event = CZ_ZMTP_MALFORMED_COMMAND_ERROR;
            return CZ_EPROTO;
        }
        if (size == 10) {
            // handleErrorReason: "3xx".."5xx" with "00" -> handshake-failed-auth event
            const char a = (char)m[7], b = (char)m[8], d = (char)m[9];
            if (b == '0' && d == '0' && a >= '3' && a <= '5') {
                *auth_status = (a - '0') * 100;
            } else {
                *event = CZ_ZAP_MALFORMED_REPLY;
                return CZ_EPROTO;
            }
        }
    }
    return CZ_OK;
}

}  // namespace czi
