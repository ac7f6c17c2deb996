"""Builds the plugin adapter library and its test driver with g++ against the stub ROS headers
(in-container check; a ROS host builds the same sources with catkin, see CMakeLists.txt)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
LIB = os.path.join(HERE, "libtraversability_estimation_filters.so")
TEST = os.path.join(HERE, "plugin_chain_test")
RADIUS_TEST = os.path.join(HERE, "plugin_radius_test")
PATHS_TEST = os.path.join(HERE, "plugin_paths_test")
IMAGE_TEST = os.path.join(HERE, "plugin_image_test")
OUTPUT_TEST = os.path.join(HERE, "plugin_output_test")
EXPRESSION_TEST = os.path.join(HERE, "plugin_expression_test")
SUBMAP_TEST = os.path.join(HERE, "plugin_submap_test")
MEDIAN_TEST = os.path.join(HERE, "plugin_median_test")
RADIUS_FILTER_TEST = os.path.join(HERE, "plugin_radius_filter_test")
WINDOW_EXPRESSION_TEST = os.path.join(HERE, "plugin_window_expression_test")
RASTER_TEST = os.path.join(HERE, "plugin_raster_test")
MOVE_TEST = os.path.join(HERE, "plugin_move_test")
SRCS = ["src/DeviceMap.cpp", "src/SlopeFilter.cpp", "src/StepFilter.cpp", "src/RoughnessFilter.cpp",
        "src/FusedChainFilter.cpp", "src/SurfaceNormalsFilter.cpp", "src/MedianFillFilter.cpp", "src/MeanInRadiusFilter.cpp", "src/MinInRadiusFilter.cpp", "src/SlidingWindowMathExpressionFilter.cpp", "src/TraversabilityMap.cpp", "stubs/pluginlib/registry.cpp"]


def build(verbose=False):
    inc = ["-I" + os.path.join(HERE, "include"), "-I" + os.path.join(HERE, "stubs"), "-I" + os.path.join(ROOT, "include")]
    common = ["g++", "-std=c++14", "-O2", "-fPIC", "-Wall", "-Wextra"] + inc
    cmd = common + ["-shared"] + [os.path.join(HERE, s) for s in SRCS] + [
        "-L" + PKG, "-ltravgpu", "-Wl,-rpath," + PKG, "-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    cmd = common + ["-I" + os.path.join(ROOT, "oracle"), os.path.join(HERE, "test", "plugin_chain_test.cpp"),
                    "-L" + HERE, "-ltraversability_estimation_filters", "-L" + os.path.join(ROOT, "oracle"), "-lte_oracle",
                    "-Wl,-rpath," + HERE, "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-Wl,-rpath," + PKG,
                    "-Wl,--no-as-needed", "-o", TEST]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # the Step and Roughness plugins at radii above 32 cells (tests/test_plugins_radius.py)
    cmd = cmd[:cmd.index(TEST)] + [RADIUS_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_chain_test.cpp"))] = os.path.join(HERE, "test", "plugin_radius_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # TraversabilityMap::setPathCheckOnDemand (tests/test_plugins_paths_radius.py)
    cmd = cmd[:cmd.index(RADIUS_TEST)] + [PATHS_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_radius_test.cpp"))] = os.path.join(HERE, "test", "plugin_paths_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # TraversabilityMap::setElevationFromImage (tests/test_plugins_image.py)
    cmd = cmd[:cmd.index(PATHS_TEST)] + [IMAGE_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_paths_test.cpp"))] = os.path.join(HERE, "test", "plugin_image_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # TraversabilityMap::getOccupancyGrid / getPointCloud (tests/test_plugins_output.py)
    cmd = cmd[:cmd.index(IMAGE_TEST)] + [OUTPUT_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_image_test.cpp"))] = os.path.join(HERE, "test", "plugin_output_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # FusedChainFilter with an `expression` parameter (tests/test_plugins_expression.py)
    cmd = cmd[:cmd.index(OUTPUT_TEST)] + [EXPRESSION_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_output_test.cpp"))] = os.path.join(HERE, "test", "plugin_expression_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # TraversabilityMap::getTraversabilityMap(position, length, layers, message) (tests/test_plugins_submap.py)
    # (the driver parses the message with te_msg_parse / te_msg_layer itself: it names libtravgpu.so on its own line)
    cmd = cmd[:cmd.index("-o")] + ["-L" + PKG, "-ltravgpu", "-o", SUBMAP_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_expression_test.cpp"))] = os.path.join(HERE, "test", "plugin_submap_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # traversabilityFilters/MedianFillFilter and TraversabilityMap::setFillHoles (tests/test_plugins_median.py)
    cmd = cmd[:cmd.index("-o")] + ["-o", MEDIAN_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_submap_test.cpp"))] = os.path.join(HERE, "test", "plugin_median_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # traversabilityFilters/MeanInRadiusFilter, MinInRadiusFilter and TraversabilityMap::setSmoothElevation (tests/test_plugins_radius_filter.py)
    cmd = cmd[:cmd.index("-o")] + ["-o", RADIUS_FILTER_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_median_test.cpp"))] = os.path.join(HERE, "test", "plugin_radius_filter_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # traversabilityFilters/SlidingWindowMathExpressionFilter (tests/test_plugins_window_expression.py)
    cmd = cmd[:cmd.index("-o")] + ["-o", WINDOW_EXPRESSION_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_radius_filter_test.cpp"))] = os.path.join(HERE, "test", "plugin_window_expression_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # SurfaceNormalsFilter and FusedChainFilter with `algorithm: raster` (tests/test_plugins_raster.py)
    cmd = cmd[:cmd.index("-o")] + ["-o", RASTER_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_window_expression_test.cpp"))] = os.path.join(HERE, "test", "plugin_raster_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # TraversabilityMap::moveMap (tests/test_plugins_move.py)
    cmd = cmd[:cmd.index("-o")] + ["-o", MOVE_TEST]
    cmd[cmd.index(os.path.join(HERE, "test", "plugin_raster_test.cpp"))] = os.path.join(HERE, "test", "plugin_move_test.cpp")
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB, TEST


if __name__ == "__main__":
    print(build(verbose=True))
