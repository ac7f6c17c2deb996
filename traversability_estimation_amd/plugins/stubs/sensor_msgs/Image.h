// stand-in for sensor_msgs/Image (msg/Image.msg): plain data, real member names
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <geometry_msgs/msgs.h>

namespace sensor_msgs {
struct Image {
  std_msgs::Header header;
  uint32_t height = 0, width = 0;
  std::string encoding;
  uint8_t is_bigendian = 0;
  uint32_t step = 0;  // bytes per image row
  std::vector<uint8_t> data;
};
}  // namespace sensor_msgs
