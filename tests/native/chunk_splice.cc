// Stand-alone check (own main; built with -fsanitize=address,undefined by
// tests/unit/test_native_chunk_splice.py) of two buffer paths of kube-lite's watch delivery
// and commit:
//  * http::ResponseWriter::write_framed_chunk puts the same bytes on the wire as
//    write_chunk, from the caller's buffer, for sizes around every width of the chunk-size
//    line, with one buffer reused across chunks;
//  * apiserver::splice_rv replaces the resourceVersion placeholder (and an older version's
//    digits) in place for 1, 7 and 20 digits, without reallocating a reserved buffer.
#include <sys/socket.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "apiserver/rv_splice.h"
#include "core/cancel.h"
#include "core/http.h"
#include "core/net.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// One end of a connected stream pair with a thread that collects what the other end writes.
struct Wire {
  std::unique_ptr<bgc::net::TcpStream> tx;
  std::string received;
  std::thread reader;
  Wire() {
    int fds[2];
    if (::socketpair(AF_UNIX, SOCK_STREAM, 0, fds) != 0) std::abort();
    tx = std::make_unique<bgc::net::TcpStream>(fds[0]);
    reader = std::thread([this, fd = fds[1]] {
      bgc::net::TcpStream rx(fd);
      char buf[65536];
      while (true) {
        const ssize_t n = rx.read_some(buf, sizeof(buf), 10000);
        if (n <= 0) break;
        received.append(buf, static_cast<size_t>(n));
      }
    });
  }
  std::string finish() {
    tx.reset();  // closes: the reader sees EOF
    reader.join();
    return received;
  }
};

std::string payload(size_t n, unsigned seed) {
  std::string s(n, '\0');
  for (size_t i = 0; i < n; ++i) s[i] = static_cast<char>('a' + (i * 7 + seed) % 26);
  if (n) s[n - 1] = '\n';
  return s;
}

void chunk_writer() {
  const std::vector<size_t> sizes = {1, 2, 15, 16, 17, 255, 256, 4095, 4096, 65535, 65536, (1u << 20) + 3, 0, 5};
  const bgc::CancelToken stop;
  Wire framed, copied;
  {
    bgc::http::ResponseWriter wf(framed.tx.get(), false, stop), wc(copied.tx.get(), false, stop);
    CHECK(wf.start_chunked(200, "application/json"));
    CHECK(wc.start_chunked(200, "application/json"));
    std::string buf;  // the caller's buffer, reused: cleared, capacity kept
    unsigned seed = 0;
    for (size_t n : sizes) {
      const std::string data = payload(n, ++seed);
      buf.clear();
      buf.append(bgc::http::ResponseWriter::kChunkHeaderRoom, ' ');
      buf += data;
      CHECK(wf.write_framed_chunk(buf));
      CHECK(wc.write_chunk(data));
    }
    std::string only_room(bgc::http::ResponseWriter::kChunkHeaderRoom, ' ');
    CHECK(wf.write_framed_chunk(only_room));  // no data: nothing is written
    std::string shorter(3, ' ');
    CHECK(wf.write_framed_chunk(shorter));
    wf.end_chunked();
    wc.end_chunked();
  }
  const std::string a = framed.finish(), b = copied.finish();
  CHECK(a == b);
  // and the stream is what the sizes say: a head, then size CRLF data CRLF per chunk, then 0
  size_t at = a.find("\r\n\r\n");
  CHECK(at != std::string::npos);
  at += 4;
  unsigned seed = 0;
  for (size_t n : sizes) {
    const std::string data = payload(n, ++seed);
    if (n == 0) continue;
    char hdr[32];
    const int h = std::snprintf(hdr, sizeof(hdr), "%zx\r\n", n);
    CHECK(a.compare(at, static_cast<size_t>(h), hdr) == 0);
    at += static_cast<size_t>(h);
    CHECK(a.compare(at, n, data) == 0);
    at += n;
    CHECK(a.compare(at, 2, "\r\n") == 0);
    at += 2;
  }
  CHECK(a.substr(at) == "0\r\n\r\n");
}

void rv_splice() {
  using bgc::apiserver::kRvSpliceSlack;
  using bgc::apiserver::splice_rv;
  const std::string head = "{\"type\":\"ADDED\",\"object\":{\"metadata\":{\"name\":\"x\",\"resourceVersion\":\"";
  const std::string placeholder = "\\u0001rv\\u0001";  // as the dumped line holds it
  const std::string tail = "\",\"uid\":\"u\"},\"spec\":{\"k\":\"" + std::string(3000, 'v') + "\"}}}\n";
  for (const std::string& digits : {std::string("7"), std::string("1234567"), std::string("18446744073709551615")}) {
    CHECK(digits.size() == 1 || digits.size() == 7 || digits.size() == 20);
    // the commit: placeholder -> digits, in a buffer reserved with the slack
    std::string line;
    line.reserve(head.size() + placeholder.size() + tail.size() + kRvSpliceSlack);
    line += head;
    line += placeholder;
    line += tail;
    const char* before = line.data();
    splice_rv(line, head.size(), placeholder.size(), digits);
    CHECK(line == head + digits + tail);
    CHECK(line.data() == before);  // in place
    // a deletion: an older version's digits -> the new ones, shorter, equal and longer
    for (const std::string& old_digits : {std::string("9"), std::string("7654321"), std::string("18446744073709551614")}) {
      std::string del;
      del.reserve(head.size() + old_digits.size() + tail.size() + kRvSpliceSlack);
      del += head;
      del += old_digits;
      del += tail;
      before = del.data();
      splice_rv(del, head.size(), old_digits.size(), digits);
      CHECK(del == head + digits + tail);
      CHECK(del.data() == before);
    }
    // without the reserve it still gives the right text (the buffer may move)
    std::string tight = head + "1" + tail;
    tight.shrink_to_fit();
    splice_rv(tight, head.size(), 1, digits);
    CHECK(tight == head + digits + tail);
  }
}

}  // namespace

int main() {
  chunk_writer();
  rv_splice();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("ok");
  return 0;
}
