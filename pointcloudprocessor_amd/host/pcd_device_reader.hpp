// pcd_device_reader.hpp -- loadPCDFile of a DATA ascii file with its rows parsed on the device (pcp_ascii_parse; DESIGN.md
// "Device PCD reader", DR7 and DR8).  The header is read by pcd_io.hpp's readPCDHeader, the file's bytes are read on this
// thread -- before the device is asked for, so a context that is still coming up on its own thread comes up meanwhile -- and
// go to the device window by window until POINTS rows are in.  A file the device reader does not take (a bad row, fewer rows
// than POINTS, x / y / z that are not 4-byte floats, DATA other than ascii, a header loadPCDFile refuses) is left to the host
// reader WHOLE: the caller calls loadPCDFile, so the program's behaviour on any file is the host reader's.
#pragma once

#include <fstream>
#include <memory>
#include <string>

#include "pcd_io.hpp"
#include "pcp_shim.hpp"

namespace pcp_amd {

struct DeviceReadResult {
  bool loaded = false;  // cloud holds the file's POINTS rows, bit for bit loadPCDFile's
  std::string why;      // not loaded: what to say about it (names the row); empty when there is nothing to say (the file is
                        // not ASCII, or the host reader will refuse it by itself)
};

// bytes per pcp_ascii_parse call (the call takes up to 2^31 - 1)
constexpr int64_t kDeviceReaderWindow = int64_t(1) << 30;

// device(): returns the Device & to parse on; called once, after the file's bytes are in memory
template <class GetDevice>
inline DeviceReadResult loadPCDFileDevice(const std::string &path, GetDevice &&device, XYZICloud &cloud) {
  DeviceReadResult res;
  std::ifstream in(path, std::ios::binary);
  if (!in) return res;
  PcdHeader head;
  if (readPCDHeader(in, head) == -1) return res;
  if (head.data_mode != "ascii") return res;
  int32_t columns = 0, col[4] = {-1, -1, -1, -1};
  for (size_t k = 0; k < head.fields.size(); ++k) {
    const int f = static_cast<int>(k);
    if (f == head.ix) col[0] = columns;
    if (f == head.iy) col[1] = columns;
    if (f == head.iz) col[2] = columns;
    if (f == head.ii) col[3] = columns;
    if (head.fields[k].count < 0 || head.fields[k].count > 64) return res;
    columns += head.fields[k].count;
  }
  if (columns < 1 || columns > 64 || col[0] >= columns || col[1] >= columns || col[2] >= columns || col[3] >= columns) {
    res.why = "a row of " + std::to_string(columns) + " columns (row 0)";
    return res;
  }
  const std::streamoff begin = in.tellg();
  in.seekg(0, std::ios::end);
  const std::streamoff end = in.tellg();
  if (begin < 0 || end < begin) return res;
  const int64_t bytes = static_cast<int64_t>(end - begin);
  std::unique_ptr<char[]> text(new char[static_cast<size_t>(bytes) + 1]);
  in.seekg(begin);
  in.read(text.get(), static_cast<std::streamsize>(bytes));
  if (in.gcount() != static_cast<std::streamsize>(bytes)) return res;
  const int64_t points = static_cast<int64_t>(head.points);
  cloud.resize(head.points);
  Device &dev = device();
  int64_t have = 0, pos = 0;
  while (have < points) {
    const int64_t len = std::min(bytes - pos, kDeviceReaderWindow);
    const bool final_window = pos + len == bytes;
    const Device::ParsedRows r = dev.parseAscii(text.get() + pos, len, columns, col, final_window, points - have, cloud.x.data() + have,
                                                cloud.y.data() + have, cloud.z.data() + have, cloud.intensity.data() + have);
    have += r.rows;
    pos += r.consumed;
    if (r.bad_row >= 0) {
      res.why = "row " + std::to_string(have) + " is not plain decimal text";
      return res;
    }
    if (have < points && (final_window || r.consumed == 0)) {  // the text is used up (or holds a row longer than a window)
      res.why = std::to_string(have) + " rows, POINTS " + std::to_string(points) + " (row " + std::to_string(have) + " is missing)";
      return res;
    }
  }
  res.loaded = true;
  return res;
}

}  // namespace pcp_amd
