// cz_hs_parse.h -- the host-only parsers of the CURVE handshake: command names, framing checks, the
// ERROR command and the metadata block.  One copy, called by the per-connection state machine
// (cz_curve_hs.cpp), the batched acceptor (cz_acceptor.cpp) and the batched connector
// (cz_connector.cpp), so the three cannot drift apart.  No HIP here: cz_hs_parse.cpp also compiles
// on its own for the CPU, which is how tools/con_parse_fuzz.cpp runs it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

namespace czi {

typedef std::vector<std::pair<std::string, std::vector<uint8_t>>> Props;
int sock_types();  // number of ZMQ_* socket types (valid types are 0 .. sock_types() - 1)
bool compatible(int self, const std::string &peer);                   // Sockets.compatible
bool starts_with(const uint8_t *m, uint64_t size, const char *data);  // Msgs.startsWith(msg, data, true)
uint64_t get_be64(const uint8_t *p);
void put_be64(uint8_t *p, uint64_t v);
// Metadata.read + Mechanism.parseMetadata's Socket-Type check: CZ_OK / CZ_EPROTO / CZ_EINVAL
int parse_metadata(const uint8_t *buf, uint64_t len, int self_type, Props *out);
std::vector<uint8_t> zmtp_metadata(int socket_type, const uint8_t *identity, size_t identity_len);

// ---- the client's side of processHandshakeCommand (CurveClientMechanism.java:105-124) ----
enum ClientCommand { CLIENT_CMD_WELCOME, CLIENT_CMD_READY, CLIENT_CMD_ERROR, CLIENT_CMD_UNKNOWN };
// which of the three commands a client takes `m` for, by its name
ClientCommand client_command(const uint8_t *m, uint64_t size);
// processWelcome's and processReady's size checks, before any box is touched: 0, or the
// ZMQ_PROTOCOL_ERROR_* event (a READY box over 16 + 16 + 256 bytes, which the reference's fixed
// buffer would throw on, is malformed here)
int welcome_framing(uint64_t size);
int ready_framing(uint64_t size);
// Mechanism.parseErrorMessage + handleErrorReason on an ERROR command: CZ_OK (*auth_status = 300 /
// 400 / 500 when the reason is such a status code, else untouched) or CZ_EPROTO with *event set
int parse_error_command(const uint8_t *m, uint64_t size, int *auth_status, int *event);

}  // namespace czi
