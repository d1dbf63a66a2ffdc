// voxelapp_headless.cpp -- the call sequence of the reference's VoxelApp/main.cu against the GPUDDA facade,
// without SDL2: build the world, build the brickmap, upload, set the environment, then per frame
// GetDirections + RenderScreen + device->host copy of the framebuffer (main.cu:18-69,165-167).  The fly camera
// is a scripted path instead of keyboard/mouse input; the last frame is written as raw BGRA and as a PPM.
//
//   voxelapp_headless [world_edge=256] [frames=2] [out_prefix=frame] [width=320] [height=180] [shaded=0]
//                     [camera_path_file] [dump_every_frame=0] [views_per_launch=1] [frames_in_flight=1] [device_world=XxYxZ]
//                     [edit_script] [walk=0]
//
// shaded: 0 = the checked-in debug view, 1 = shaded with shadow + 1 bounce sample, checkerboard on, 2 = the same with the
// checkerboard off (whole frames).  frames_in_flight=2 renders through Graphics::RenderScreenAsync / WaitFrame: frame k+1 is
// launched before frame k is copied to the host, on two alternating device buffers (use shaded=2: under checkerboard a
// frame needs its predecessor's buffer).  device_world=8192x512x8192 builds the brickmap on the device in one step
// (VoxelRaytracer3D::BuildProceduralWorld) instead of CreateVoxels + GenerateLowresVoxelBuffer, whose dense bit array
// the reference cannot index beyond 2^32 voxels; `world_edge` then only scales the default camera.  A '-' skips
// camera_path_file.  The run ends with the rays traced and the Mrays/s over the frame loop.

// camera_path_file replaces the fixed camera: one frame per line, "x y z eulerX eulerY eulerZ" (voxels, radians;
// '#' starts a comment); `frames` is then the number of lines.  With dump_every_frame=1 each frame is also written
// as <out_prefix>_NNNN.ppm (under checkerboard rendering a frame keeps the other half of the previous one).
// views_per_launch > 1 renders that many poses per launch through Graphics::RenderScreens (no checkerboard then).
// edit_script (voxel editing, VoxelRaytracer3D::EditVoxels): one op per line, "frame kind value ax ay az bx by bz" --
// kind 0 = box a..b (inclusive voxels), 1 = sphere of centre a and radius bx (by = bz = 0); value 1 = set, 0 = clear --
// applied in file order before that frame is rendered ('#' starts a comment; with views_per_launch > 1, before the launch
// that holds the frame).  A '-' skips it.  Two more kinds copy and paste (VoxelRaytracer3D::ReadRegion / StampVoxels):
// kind 2 = copy the box of origin a and dims b into clipboard slot `value`; kind 3 = paste clipboard slot `value` with its
// voxel (0,0,0) at a, in mode bx (0 = replace, 1 = union, 2 = subtract; by = bz = 0).  Kind 4 collapses the floating
// islands of the box of origin a and dims b (VoxelRaytracer3D::FindIslands, anchored on the box's six faces and world y = 0,
// then a subtract stamp of them): one line "collapse before frame N: C components, I islands, V island voxels, ..." with the
// stamp's brick counts.  A dig that severs an overhang, then a collapse around it, removes the overhang.  Kind 5 computes a
// navigation field over the box of origin a and dims b (VoxelRaytracer3D::NavField, the default agent width 1, height 2,
// climb 1, drop 3) with one goal, the cell that holds frame N's camera position (floor of each coordinate), and prints one
// line "nav frame N nodes .. reached .. levels .. max_dist ..".  Kind 6 computes the exact distance field of the box of
// origin a and dims b (VoxelRaytracer3D::DistanceField) within the radius |value|, to the nearest solid voxel when value > 0
// and to the nearest empty voxel when value < 0, and prints one line "dist frame N zero .. near .. far .. max_d2 .. sum_d2 ..".
// Kind 7 stamps a built-in mesh (VoxelRaytracer3D::StampMesh, union): an octahedron generated here, its centre on the centre of
// voxel a, its radius bx voxels (by = bz = 0), voxelized in the modes `value` (1 = surface, 2 = solid, 3 = both), and prints one
// line "mesh before frame N: T triangles, S set voxels, ... bricks touched, ... created".
// Kind 8 extracts the surface of the box of origin a and dims b (VoxelRaytracer3D::ExtractSurface, with triangles) in the mode
// `value` (0 = VXRT_SURF_CAP, 1 = VXRT_SURF_OPEN) and prints one line "surface frame N solid .. faces .. quads .. tris ..",
// then one line "surface hash frame N quads .. vertices .. triangles .." with the 64-bit FNV-1a hash of each array's bytes.
// Kind 9 downsamples the box of origin a and cell dims b (VoxelRaytracer3D::DownsampleRegion, with counts) at shift
// `value & 7` and threshold `value >> 3` and prints one line "lod frame N shift .. threshold .. set .. empty .. full .. mixed ..
// max .. solid ..", then one line "lod hash frame N bits .. counts .." with the 64-bit FNV-1a hash of each array's bytes.
// Kind 10 computes the light field of the box of origin a and dims b (VoxelRaytracer3D::LightField) in the channels
// `value & 3` (1 = sky, 2 = block), with one emitter of level 15 in the cell that holds frame N's camera position when the
// block channel is set, and prints one line "light frame N solid .. exposed .. sky_sum .. block_sum .. used ..", then one
// line "light hash frame N levels .." with the 64-bit FNV-1a hash of the level bytes.
// Kind 11 drops the floating islands of the box of origin a and dims b instead of deleting them (VoxelRaytracer3D::DropIslands,
// anchored as kind 4: each island falls along -y until it lands, lowest first) and prints one line "drop before frame N: I
// islands, V island voxels, M moved, max_fall F, sum_contact C", then one line "drop hash frame N rows .." with the 64-bit
// FNV-1a hash of the rows' bytes (id, voxels, travel, contact: 16 bytes each, in dropping order).
// A line "frame denoise iterations color_scale" switches the frame denoiser on from that frame (vxrt_frame_guides +
// vxrt_denoise_frame; "frame denoise 0" switches it off again): such a frame is rendered through vxrt_render with the colour
// and hit-index AOVs, its guide keys are computed and the filtered colour replaces the frame -- the dumped PPMs are the
// denoised frames -- with one line "denoise frame N iterations .. color_scale .. hit .. faces .. hash .." (hit pixels, distinct
// keys, the 64-bit FNV-1a hash of the BGRA frame).  Whole frames only: shaded=0 or 2, views_per_launch=1, frames_in_flight=1.
// The AOVs, the keys and the workspace are allocated once.
// A line "frame temporal on|off [max_history]" switches the temporal filter on or off from that frame (vxrt_reproject_frame;
// max_history defaults to 32): such a frame is rendered with the AOVs, its guide keys are computed and the frame history of
// the previous frame is reprojected from that frame's pose into this one's -- before the denoiser when both are on, which
// then filters the accumulated mean -- with one line "temporal frame N max_history .. hit .. reused .. offscreen ..
// rejected ..".  The history starts anew at the first such frame and after every frame with an edit line.  The same
// restrictions as for the denoiser; two history and two key buffers are allocated once.
// A line "frame lit ox oy oz dx dy dz sky_floor [ex ey ez level]..." switches the light on frames on from that frame
// (vxrt_light_frame; "frame lit off" switches it off again): at that frame the light field of the box of origin (ox, oy, oz)
// and dims (dx, dy, dz) is computed once, in both channels and with the given emitters (vxrt_light_field_host), and from then
// on every frame is rendered with the AOVs, its guide keys are computed and, as the last stage after the temporal filter and
// the denoiser, every hit pixel is relit with both flags, outside_level 0xF0, the block colour (1, 0.8, 0.5) and the occlusion
// curve (0.4, 0.6, 0.8, 1) -- the dumped PPMs are the lit frames -- with one line "lit frame N hit .. in_box .. occluded ..
// dark ..".  The same restrictions as for the denoiser.
// A line "frame materials" switches the voxel materials on from that frame (vxrt_material_frame; "frame materials off" switches
// them off again): after the denoiser and before the light, every hit pixel's colour is multiplied with the albedo of the voxel
// it shows -- five built-in materials in two altitude bands (grass over dirt over stone; from 5/8 of the world's height snow
// over sand over stone), each with a tile of an 8 x 8 atlas made on the host from an integer hash (grass has a side tile of
// its own) -- with one line "materials frame N hit .. painted .. top .. textured ..".  The dumped PPMs are the coloured frames.
// The same restrictions as for the denoiser.
// A line "frame sky [clouds]" switches the sky on from that frame (vxrt_sky_frame; "frame sky off" switches it off again): as the
// last stage, after the light, every pixel that misses the world gets a sky -- a built-in daytime preset whose sun stands in the
// environment's light direction, with "clouds" also a layer of clouds at twice the world's height -- and every hit pixel fades
// into it with its distance, with one line "sky frame N miss .. ground .. sun .. cloud .. fogged ..".  The dumped PPMs are the
// finished frames.  The same restrictions as for the denoiser.
// A line "frame rule x0 y0 z0 x1 y1 z1 n6|n18|n26 born_hex survive_hex iterations box|world" applies a neighbour-count rule
// (VoxelRaytracer3D::ApplyRule) to the box of the inclusive corners (x0, y0, z0) .. (x1, y1, z1) -- born_hex / survive_hex: bit
// c set = an empty voxel is born / a solid voxel survives with c solid neighbours -- stamps the result (replace) and prints one
// line "rule before frame N: before .. after .. born .. died .. changed_last .. box <lo x3> <hi x3>, ... bricks touched".
// "frame smooth x0 y0 z0 x1 y1 z1 iterations" is the shorthand for the majority rule on the box alone
// (VoxelRaytracer3D::SmoothVoxels), with the same line.  Both are applied in file order with the edit lines.
// A line "frame loose sand|water x0 y0 z0 x1 y1 z1 sx0 sy0 sz0 sx1 sy1 sz1 steps wall|open" turns the solid voxels of the source
// box (sx0, sy0, sz0) .. (sx1, sy1, sz1) loose inside the box (x0, y0, z0) .. (x1, y1, z1) (inclusive corners) and makes exactly
// `steps` steps with them (VoxelRaytracer3D::SettleVoxels without the early stop), stamps them back and prints one line "loose
// before frame N: in .. start .. after .. fell_last .. slid_last .. spread_last .. box <lo x3> <hi x3>, ... bricks touched" (the
// summary of the last call of at most VXRT_LOOSE_MAX_STEPS steps).
// "frame turn axis quarter_turns [slot=0]" and "frame mirror axis [slot=0]" re-orient the clipboard slot a copy line filled
// (vxrt_orientation_rotation / a flip of one axis, then vxrt_transform_stamp): the slot's bits are kept on the device from the
// first such line on, each line transforms them into a second device buffer and swaps the two, and a following paste pastes
// the turned stamp, its voxel (0,0,0) at the paste's a.  One line "turn before frame N: slot S, dims X Y Z, V voxels, box
// <lo x3> <hi x3>, hash H" (the 64-bit FNV-1a hash of the turned words; "mirror before frame ..." for a mirror line).
// walk=1 (box collision, VoxelRaytracer3D::MoveBoxes): the camera is a body of half-extents (2, 6, 2) voxels that starts at
// the first frame's pose; every frame, after that frame's edits, it moves toward the frame's pose -- delta = pose - centre,
// each axis clamped to VXRT_BODY_MAX_DELTA, in the order y, x, z -- instead of jumping there, and the frame renders from the
// body's centre.  One line per frame: "walk frame N lo <%a x3> hi <%a x3> flags F".
#include "../include/GPUDDA/Renderer.h"
#include "../include/GPUDDA/VoxelWorldBuilder.h"
#include "../include/vxrt.h"

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace GPUDDA;
using namespace GPUDDA::Graphics;

int main(int argc, char** argv)
{
    const unsigned edge = argc > 1 ? (unsigned)atoi(argv[1]) : 256u;
    const int frames = argc > 2 ? atoi(argv[2]) : 2;
    const std::string prefix = argc > 3 ? argv[3] : "frame";
    const uint32_t width = argc > 4 ? (uint32_t)atoi(argv[4]) : 320u, height = argc > 5 ? (uint32_t)atoi(argv[5]) : 180u;
    const bool shaded = argc > 6 && atoi(argv[6]) != 0;
    const int shade_mode = argc > 6 ? atoi(argv[6]) : 0;
    const std::string path_file = (argc > 7 && std::string(argv[7]) != "-") ? argv[7] : "";
    const bool dump_all = argc > 8 && atoi(argv[8]) != 0;
    const int batch = argc > 9 ? atoi(argv[9]) : 1;
    const int in_flight = argc > 10 ? atoi(argv[10]) : 1;
    unsigned wx = 0, wy = 0, wz = 0;
    if (argc > 11 && std::sscanf(argv[11], "%ux%ux%u", &wx, &wy, &wz) != 3) {
        std::cerr << "device_world must look like 8192x512x8192" << std::endl;
        return 2;
    }

    struct EditLine {
        int frame;
        vxrt_edit_op op;  // kind 12: a rule line (a = the box's origin, b = its dims; value 1: the smooth shorthand)
                          // kind 13 / 14: a turn / mirror line (value = the slot, a[0] = the axis, a[1] = the quarter turns)
                          // kind 15: a loose line (a, b = the box's origin and dims; value = the material)
        vxrt_rule rule;
        int32_t src_o[3], src_d[3], steps, edge;  // kind 15: the source box, the steps and the edge mode
    };
    std::vector<EditLine> edits;
    struct DenoiseLine {
        int frame, iterations;
        float color_scale;
    };
    std::vector<DenoiseLine> denoise_lines;
    struct TemporalLine {
        int frame, max_history;
        bool on;
    };
    std::vector<TemporalLine> temporal_lines;
    struct LitLine {
        int frame;
        bool on;
        int32_t origin[3], dims[3];
        float sky_floor;
        std::vector<int32_t> emitters;  // x, y, z, level each
    };
    std::vector<LitLine> lit_lines;
    struct MaterialsLine {
        int frame;
        bool on;
    };
    std::vector<MaterialsLine> materials_lines;
    struct SkyLine {
        int frame;
        bool on, clouds;
    };
    std::vector<SkyLine> sky_lines;
    if (argc > 12 && std::string(argv[12]) != "-") {
        std::ifstream in(argv[12]);
        if (!in) {
            std::cerr << "cannot open edit script " << argv[12] << std::endl;
            return 2;
        }
        std::string line;
        while (std::getline(in, line)) {
            const size_t hash = line.find('#');
            if (hash != std::string::npos)
                line.resize(hash);
            EditLine e{};
            DenoiseLine dl{0, 0, 0.0f};
            if (std::sscanf(line.c_str(), "%d denoise %d %f", &dl.frame, &dl.iterations, &dl.color_scale) >= 2) {
                denoise_lines.push_back(dl);
                continue;
            }
            TemporalLine tl{0, 32, false};
            char word[8] = "";
            if (std::sscanf(line.c_str(), "%d temporal %7s %d", &tl.frame, word, &tl.max_history) >= 2 &&
                (std::string(word) == "on" || std::string(word) == "off")) {
                tl.on = std::string(word) == "on";
                temporal_lines.push_back(tl);
                continue;
            }
            {
                MaterialsLine ml{0, true};
                char what[12] = "", arg[8] = "";
                const int got = std::sscanf(line.c_str(), "%d %11s %7s", &ml.frame, what, arg);
                if (got >= 2 && std::string(what) == "materials") {
                    if (got == 3 && std::string(arg) != "off") {
                        std::cerr << "bad materials line: " << line << std::endl;
                        return 2;
                    }
                    ml.on = got == 2;
                    materials_lines.push_back(ml);
                    continue;
                }
            }
            {
                SkyLine sl{0, true, false};
                char what[12] = "", arg[8] = "";
                const int got = std::sscanf(line.c_str(), "%d %11s %7s", &sl.frame, what, arg);
                if (got >= 2 && std::string(what) == "sky") {
                    if (got == 3 && std::string(arg) != "off" && std::string(arg) != "clouds") {
                        std::cerr << "bad sky line: " << line << std::endl;
                        return 2;
                    }
                    sl.on = !(got == 3 && std::string(arg) == "off");
                    sl.clouds = got == 3 && std::string(arg) == "clouds";
                    sky_lines.push_back(sl);
                    continue;
                }
            }
            {
                std::istringstream words(line);
                LitLine ll{};
                std::string word2, first;
                if (words >> ll.frame >> word2 && word2 == "lit") {
                    std::streampos at = words.tellg();
                    if (words >> first && first == "off") {
                        lit_lines.push_back(ll);
                        continue;
                    }
                    words.clear();
                    words.seekg(at);
                    if (words >> ll.origin[0] >> ll.origin[1] >> ll.origin[2] >> ll.dims[0] >> ll.dims[1] >> ll.dims[2] >> ll.sky_floor) {
                        int32_t e[4];
                        while (words >> e[0] >> e[1] >> e[2] >> e[3])
                            ll.emitters.insert(ll.emitters.end(), e, e + 4);
                        ll.on = true;
                        lit_lines.push_back(ll);
                        continue;
                    }
                    std::cerr << "bad lit line: " << line << std::endl;
                    return 2;
                }
            }
            {
                int axis = 0, turns = 0, slot = 0;
                const bool turn = std::sscanf(line.c_str(), "%d turn %d %d %d", &e.frame, &axis, &turns, &slot) >= 3;
                const bool mirror = !turn && std::sscanf(line.c_str(), "%d mirror %d %d", &e.frame, &axis, &slot) >= 2;
                if (turn || mirror) {
                    e.op.kind = turn ? 13 : 14;
                    e.op.value = slot;
                    e.op.a[0] = axis;
                    e.op.a[1] = turns;
                    edits.push_back(e);
                    continue;
                }
            }
            {
                int c[12], steps = 0;
                char mat[8] = "", edge[8] = "";
                if (std::sscanf(line.c_str(), "%d loose %7s %d %d %d %d %d %d %d %d %d %d %d %d %d %7s", &e.frame, mat, &c[0], &c[1], &c[2], &c[3],
                                &c[4], &c[5], &c[6], &c[7], &c[8], &c[9], &c[10], &c[11], &steps, edge) == 16) {
                    const std::string m(mat), ed(edge);
                    if ((m != "sand" && m != "water") || (ed != "wall" && ed != "open")) {
                        std::cerr << "edit script: cannot read \"" << line << "\"" << std::endl;
                        return 2;
                    }
                    e.op.kind = 15;
                    e.op.value = m == "water" ? VXRT_LOOSE_WATER : VXRT_LOOSE_SAND;
                    for (int k = 0; k < 3; ++k) {
                        e.op.a[k] = c[k];
                        e.op.b[k] = c[3 + k] - c[k] + 1;
                        e.src_o[k] = c[6 + k];
                        e.src_d[k] = c[9 + k] - c[6 + k] + 1;
                    }
                    e.steps = steps;
                    e.edge = ed == "open" ? VXRT_LOOSE_OPEN : VXRT_LOOSE_WALL;
                    edits.push_back(e);
                    continue;
                }
            }
            {
                int c[6], iterations = 1;
                char nb[8] = "", scope[8] = "";
                unsigned born = 0, survive = 0;
                const bool rule = std::sscanf(line.c_str(), "%d rule %d %d %d %d %d %d %7s %x %x %d %7s", &e.frame, &c[0], &c[1], &c[2], &c[3],
                                              &c[4], &c[5], nb, &born, &survive, &iterations, scope) == 12;
                const bool smooth = !rule && std::sscanf(line.c_str(), "%d smooth %d %d %d %d %d %d %d", &e.frame, &c[0], &c[1], &c[2], &c[3],
                                                         &c[4], &c[5], &iterations) == 8;
                if (rule || smooth) {
                    const std::string n(nb), sc(scope);
                    if (rule && ((n != "n6" && n != "n18" && n != "n26") || (sc != "box" && sc != "world"))) {
                        std::cerr << "edit script: cannot read \"" << line << "\"" << std::endl;
                        return 2;
                    }
                    e.op.kind = 12;
                    e.op.value = smooth ? 1 : 0;
                    for (int k = 0; k < 3; ++k) {
                        e.op.a[k] = c[k];
                        e.op.b[k] = c[3 + k] - c[k] + 1;
                    }
                    e.rule.struct_size = sizeof(vxrt_rule);
                    e.rule.neighbours = n == "n6" ? VXRT_RULE_N6 : n == "n18" ? VXRT_RULE_N18 : VXRT_RULE_N26;
                    e.rule.born = born;
                    e.rule.survive = survive;
                    e.rule.iterations = iterations;
                    e.rule.scope = sc == "world" ? VXRT_RULE_WORLD : VXRT_RULE_BOX;
                    edits.push_back(e);
                    continue;
                }
            }
            if (std::sscanf(line.c_str(), "%d %d %d %d %d %d %d %d %d", &e.frame, &e.op.kind, &e.op.value, &e.op.a[0], &e.op.a[1],
                            &e.op.a[2], &e.op.b[0], &e.op.b[1], &e.op.b[2]) == 9)
                edits.push_back(e);
            else if (line.find_first_not_of(" \t\r") != std::string::npos) {
                std::cerr << "edit script: cannot read \"" << line << "\"" << std::endl;
                return 2;
            }
        }
    }

    const bool walk = argc > 13 && atoi(argv[13]) != 0;

    struct Pose {
        float3 pos, euler;
    };
    std::vector<Pose> path;
    if (!path_file.empty()) {
        std::ifstream in(path_file);
        if (!in) {
            std::cerr << "cannot open camera path " << path_file << std::endl;
            return 2;
        }
        std::string line;
        while (std::getline(in, line)) {
            const size_t hash = line.find('#');
            if (hash != std::string::npos)
                line.resize(hash);
            float v[6];
            if (std::sscanf(line.c_str(), "%f %f %f %f %f %f", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) == 6)
                path.push_back({make_float3(v[0], v[1], v[2]), make_float3(v[3], v[4], v[5])});
        }
        if (path.empty()) {
            std::cerr << "camera path " << path_file << " holds no poses" << std::endl;
            return 2;
        }
    }

    int factor = 32;
    VoxelRaytracer3D* raytracer = new VoxelRaytracer3D(1);
    auto t0 = std::chrono::high_resolution_clock::now();
    if (wx) {
        raytracer->BuildProceduralWorld(make_uint3(wx, wy, wz), factor);
        auto t1 = std::chrono::high_resolution_clock::now();
        std::cout << "World built on the device: " << std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count() << "ms" << std::endl;
    } else {
        auto buffer = CreateVoxels(make_uint3(edge, edge, edge));
        auto t1 = std::chrono::high_resolution_clock::now();
        std::cout << "Voxel generation time: " << std::chrono::duration_cast<std::chrono::milliseconds>(t1 - t0).count() << "ms" << std::endl;

        auto buffers = GenerateLowresVoxelBuffer(buffer, factor);
        auto t2 = std::chrono::high_resolution_clock::now();
        std::cout << "Buffer generation time: " << std::chrono::duration_cast<std::chrono::milliseconds>(t2 - t1).count() << "ms" << std::endl;
        delete[] buffer.grid.Raw();

        auto low_res_buffer = std::get<0>(buffers);
        auto low_res_grid_data = std::get<1>(buffers);
        auto bounds = std::get<2>(buffers);
        auto count = (size_t)low_res_buffer.dimensions[0] * low_res_buffer.dimensions[1] * low_res_buffer.dimensions[2];
        raytracer->UploadVoxelBuffer(low_res_buffer);
        raytracer->UploadVoxelBufferDatas(low_res_grid_data, count);
        raytracer->UploadVoxelBufferDataBounds(bounds, count);
        raytracer->SetFactor(factor);
    }

    float3 cam_pos = wx ? make_float3(wx * 0.5f, wy * 0.9f, wz * 0.5f) : make_float3(edge * 0.25f, edge * 0.9f, edge * 0.25f);
    float3 cam_up, cam_right, cam_forward;
    float3 cam_eular = make_float3(-0.45f, 0.7f, 0.0f);

    Environment env;
    const float inv = 1.0f / std::sqrt(3.0f);
    env.LightDirection = make_float3(1.0f * inv, 1.0f * inv, 1.0f * inv);
    env.LightColor = make_float3(2, 2, 2);
    env.AmbientColor = make_float3(0.5f, 0.5f, 0.5f);
    SetEnvironment(env);
    SetFOV(90);
    SetOrthoWindowSize(make_float2(10, 10));
    if (shaded) {  // the README screenshots' configuration; default = the checked-in debug view
        RenderSwitches s;
        s.DebugView = false;
        s.ShadowRay = true;
        s.BounceSamples = 1;
        s.Checkerboard = shade_mode != 2;
        SetRenderSwitches(s);
    }

    // the edit script's lines of frames [from, to), in file order: box / sphere ops in calls of at most VXRT_EDIT_MAX_OPS
    // ops, a copy or paste line after the ops before it
    struct Clip {
        int32_t dims[3];
        std::vector<uint32_t> bits;
        uint32_t* d_bits = nullptr;  // the same bits on the device once a turn or mirror line has used the slot
    };
    std::map<int, Clip> clipboard;
    auto apply_edits = [&](int from, int to) {
        std::vector<vxrt_edit_op> ops;
        auto flush_ops = [&]() {
            for (size_t k = 0; k < ops.size(); k += VXRT_EDIT_MAX_OPS) {
                const size_t n = ops.size() - k < VXRT_EDIT_MAX_OPS ? ops.size() - k : VXRT_EDIT_MAX_OPS;
                vxrt_edit_stats st{};
                if (raytracer->EditVoxels(ops.data() + k, n, &st) != VXRT_OK) {
                    std::cerr << "edit before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("edit before frame %d: %zu ops, %llu bricks touched, %llu created, %llu freed\n", from, n,
                            (unsigned long long)st.bricks_touched, (unsigned long long)st.bricks_created, (unsigned long long)st.bricks_freed);
            }
            ops.clear();
        };
        for (const EditLine& e : edits) {
            if (e.frame < from || e.frame >= to)
                continue;
            if (e.op.kind == 2) {  // copy
                flush_ops();
                Clip& c = clipboard[e.op.value];
                (void)hipFree(c.d_bits);
                c.d_bits = nullptr;
                for (int k = 0; k < 3; ++k)
                    c.dims[k] = e.op.b[k];
                if (raytracer->ReadRegion(e.op.a, c.dims, c.bits) != VXRT_OK) {
                    std::cerr << "copy before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("copy before frame %d: slot %d, %zu words\n", from, e.op.value, c.bits.size());
            } else if (e.op.kind == 4) {  // collapse islands
                flush_ops();
                std::vector<uint32_t> floating;
                vxrt_island_summary sum{};
                vxrt_edit_stats st{};
                if (raytracer->FindIslands(e.op.a, e.op.b, VXRT_ISLAND_ANCHOR_FACES | VXRT_ISLAND_ANCHOR_FLOOR, floating, sum) != VXRT_OK ||
                    raytracer->StampVoxels(e.op.a, e.op.b, floating.data(), VXRT_STAMP_SUBTRACT, &st) != VXRT_OK) {
                    std::cerr << "collapse before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("collapse before frame %d: %u components, %u islands, %u island voxels, %llu bricks touched, %llu created, "
                            "%llu freed\n", from, sum.components, sum.islands, sum.island_voxels, (unsigned long long)st.bricks_touched,
                            (unsigned long long)st.bricks_created, (unsigned long long)st.bricks_freed);
            } else if (e.op.kind == 5) {  // navigation field toward the camera's cell
                flush_ops();
                const float3 cp = path.empty() ? cam_pos : path[(size_t)from].pos;
                const int32_t goal[3] = {(int32_t)std::floor(cp.x), (int32_t)std::floor(cp.y), (int32_t)std::floor(cp.z)};
                const vxrt_nav_agent agent{1, 2, 1, 3};
                std::vector<uint32_t> walkable;
                std::vector<uint8_t> next;
                vxrt_nav_summary sum{};
                if (raytracer->NavField(e.op.a, e.op.b, agent, goal, 1, 1u << 24, walkable, next, sum) != VXRT_OK) {
                    std::cerr << "nav before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("nav frame %d nodes %u reached %u levels %u max_dist %u\n", from, sum.nodes, sum.reached, sum.levels,
                            sum.max_dist_found);
            } else if (e.op.kind == 6) {  // distance field
                flush_ops();
                std::vector<uint16_t> dist2;
                vxrt_distance_summary sum{};
                const uint32_t radius = (uint32_t)std::abs((long long)e.op.value);
                if (raytracer->DistanceField(e.op.a, e.op.b, radius, e.op.value < 0 ? VXRT_DIST_TO_EMPTY : VXRT_DIST_TO_SOLID, dist2,
                                             sum) != VXRT_OK) {
                    std::cerr << "dist before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("dist frame %d zero %u near %u far %u max_d2 %u sum_d2 %llu\n", from, sum.zero, sum.near, sum.far,
                            sum.max_d2, (unsigned long long)sum.sum_d2);
            } else if (e.op.kind == 8) {  // surface extraction
                flush_ops();
                std::vector<vxrt_quad> quads;
                std::vector<int32_t> verts;
                std::vector<uint32_t> tris;
                vxrt_surface_summary sum{};
                if (raytracer->ExtractSurface(e.op.a, e.op.b, e.op.value, quads, &sum, &verts, &tris) != VXRT_OK) {
                    std::cerr << "surface before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("surface frame %d solid %u faces %u quads %u tris %zu\n", from, sum.solid, sum.faces, sum.quads,
                            tris.size() / 3);
                auto fnv = [](const void* p, size_t n) {
                    uint64_t h = 0xcbf29ce484222325ull;
                    for (size_t i = 0; i < n; ++i)
                        h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
                    return (unsigned long long)h;
                };
                std::printf("surface hash frame %d quads %016llx vertices %016llx triangles %016llx\n", from,
                            fnv(quads.data(), quads.size() * sizeof(vxrt_quad)), fnv(verts.data(), verts.size() * 4),
                            fnv(tris.data(), tris.size() * 4));
            } else if (e.op.kind == 9) {  // occupancy LOD
                flush_ops();
                std::vector<uint32_t> bits;
                std::vector<uint16_t> counts;
                vxrt_lod_summary sum{};
                const uint32_t shift = (uint32_t)e.op.value & 7u, threshold = (uint32_t)e.op.value >> 3;
                if (raytracer->DownsampleRegion(e.op.a, e.op.b, shift, threshold, bits, sum, &counts) != VXRT_OK) {
                    std::cerr << "lod before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("lod frame %d shift %u threshold %u set %u empty %u full %u mixed %u max %u solid %llu\n", from, shift,
                            threshold, sum.set, sum.empty, sum.full, sum.mixed, sum.max_count, (unsigned long long)sum.solid);
                auto fnv = [](const void* p, size_t n) {
                    uint64_t h = 0xcbf29ce484222325ull;
                    for (size_t i = 0; i < n; ++i)
                        h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
                    return (unsigned long long)h;
                };
                std::printf("lod hash frame %d bits %016llx counts %016llx\n", from, fnv(bits.data(), bits.size() * 4),
                            fnv(counts.data(), counts.size() * 2));
            } else if (e.op.kind == 10) {  // light field, one emitter in the camera's cell
                flush_ops();
                const float3 cp = path.empty() ? cam_pos : path[(size_t)from].pos;
                const uint32_t channels = (uint32_t)e.op.value & 3u;
                std::vector<int32_t> emitters;
                if (channels & VXRT_LIGHT_BLOCK)
                    emitters = {(int32_t)std::floor(cp.x), (int32_t)std::floor(cp.y), (int32_t)std::floor(cp.z), VXRT_LIGHT_MAX};
                std::vector<uint8_t> levels;
                vxrt_light_summary sum{};
                if (raytracer->LightField(e.op.a, e.op.b, emitters, channels, levels, sum) != VXRT_OK) {
                    std::cerr << "light before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("light frame %d solid %u exposed %u sky_sum %llu block_sum %llu used %u\n", from, sum.solid, sum.exposed,
                            (unsigned long long)sum.sum_sky, (unsigned long long)sum.sum_block, sum.emitters_used);
                uint64_t h = 0xcbf29ce484222325ull;
                for (size_t i = 0; i < levels.size(); ++i)
                    h = (h ^ levels[i]) * 0x100000001b3ull;
                std::printf("light hash frame %d levels %016llx\n", from, (unsigned long long)h);
            } else if (e.op.kind == 12) {  // a neighbour-count rule, or the smooth shorthand, stamped
                flush_ops();
                vxrt_rule_summary sum{};
                vxrt_edit_stats st{};
                int rc;
                if (e.op.value) {
                    rc = raytracer->SmoothVoxels(e.op.a, e.op.b, e.rule.iterations, &st, &sum);
                } else {
                    std::vector<uint32_t> bits;
                    rc = raytracer->ApplyRule(e.op.a, e.op.b, e.rule, bits, sum);
                    if (rc == VXRT_OK)
                        rc = raytracer->StampVoxels(e.op.a, e.op.b, bits.data(), VXRT_STAMP_REPLACE, &st);
                }
                if (rc != VXRT_OK) {
                    std::cerr << "rule before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("rule before frame %d: before %u after %u born %u died %u changed_last %u box %d %d %d %d %d %d, %llu bricks "
                            "touched\n", from, sum.solid_before, sum.solid_after, sum.born, sum.died, sum.changed_last, sum.changed_min[0],
                            sum.changed_min[1], sum.changed_min[2], sum.changed_max[0], sum.changed_max[1], sum.changed_max[2],
                            (unsigned long long)st.bricks_touched);
            } else if (e.op.kind == 15) {  // the source box's voxels turned loose, stepped and stamped back
                flush_ops();
                vxrt_loose_summary sum{};
                vxrt_edit_stats st{};
                if (raytracer->SettleVoxels(e.op.a, e.op.b, e.src_o, e.src_d, e.op.value, e.steps, e.edge, &sum, nullptr, &st, false) != VXRT_OK) {
                    std::cerr << "loose before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("loose before frame %d: in %u start %u after %u fell_last %u slid_last %u spread_last %u box %d %d %d %d %d %d, "
                            "%llu bricks touched\n", from, sum.loose_in, sum.loose_start, sum.loose_after, sum.fell_last, sum.slid_last,
                            sum.spread_last, sum.changed_min[0], sum.changed_min[1], sum.changed_min[2], sum.changed_max[0],
                            sum.changed_max[1], sum.changed_max[2], (unsigned long long)st.bricks_touched);
            } else if (e.op.kind == 11) {  // drop the islands
                flush_ops();
                std::vector<VoxelRaytracer3D::DroppedIsland> rows;
                if (raytracer->DropIslands(e.op.a, e.op.b, VXRT_ISLAND_ANCHOR_FACES | VXRT_ISLAND_ANCHOR_FLOOR, rows) != VXRT_OK) {
                    std::cerr << "drop before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                unsigned long long voxels = 0, contact = 0;
                unsigned moved = 0;
                int fall = 0;
                for (const auto& r : rows) {
                    voxels += r.voxels;
                    contact += r.contact;
                    moved += r.travel != 0;
                    fall = -r.travel > fall ? -r.travel : fall;
                }
                std::printf("drop before frame %d: %zu islands, %llu island voxels, %u moved, max_fall %d, sum_contact %llu\n", from,
                            rows.size(), voxels, moved, fall, contact);
                uint64_t h = 0xcbf29ce484222325ull;
                for (size_t i = 0; i < rows.size() * sizeof(rows[0]); ++i)
                    h = (h ^ ((const unsigned char*)rows.data())[i]) * 0x100000001b3ull;
                std::printf("drop hash frame %d rows %016llx\n", from, (unsigned long long)h);
            } else if (e.op.kind == 7) {  // stamp the built-in mesh
                flush_ops();
                const int32_t r = 256 * e.op.b[0], c = 128;  // mesh frame: the origin is the corner of voxel a
                const std::vector<int32_t> verts = {c + r, c, c, c - r, c, c, c, c + r, c, c, c - r, c, c, c, c + r, c, c, c - r};
                const std::vector<uint32_t> tris = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
                vxrt_edit_stats st{};
                vxrt_voxelize_summary sum{};
                if (e.op.b[0] < 1 || e.op.b[1] != 0 || e.op.b[2] != 0 ||
                    raytracer->StampMesh(verts, tris, e.op.a, e.op.value, VXRT_STAMP_UNION, &st, &sum) != VXRT_OK) {
                    std::cerr << "mesh before frame " << from << ": " << vxrt_last_error() << std::endl;
                    std::exit(3);
                }
                std::printf("mesh before frame %d: %u triangles, %u set voxels, %llu bricks touched, %llu created\n", from, sum.triangles,
                            sum.set, (unsigned long long)st.bricks_touched, (unsigned long long)st.bricks_created);
            } else if (e.op.kind == 13 || e.op.kind == 14) {  // turn or mirror the clipboard slot on the device
                flush_ops();
                const char* what = e.op.kind == 13 ? "turn" : "mirror";
                const auto it = clipboard.find(e.op.value);
                vxrt_orientation o{{0, 1, 2}, 0u};
                int32_t dd[3] = {0, 0, 0};
                bool ok = it != clipboard.end();
                if (ok && e.op.kind == 13)
                    ok = vxrt_orientation_rotation(e.op.a[0], e.op.a[1], &o) == VXRT_OK;
                else if (ok && (ok = e.op.a[0] >= 0 && e.op.a[0] <= 2))
                    o.flip = 1u << e.op.a[0];
                vxrt_transform_summary sum{};
                if (ok) {
                    Clip& c = it->second;
                    (void)vxrt_orientation_dims(&o, c.dims, dd);
                    const size_t nsrc = c.bits.size(), ndst = (size_t)vxrt_region_words(dd);
                    uint32_t* d_turned = nullptr;
                    vxrt_transform_summary* d_sum = nullptr;
                    std::vector<uint32_t> turned(ndst);
                    ok = (c.d_bits || (hipMalloc((void**)&c.d_bits, nsrc * 4) == hipSuccess &&
                                       hipMemcpy(c.d_bits, c.bits.data(), nsrc * 4, hipMemcpyHostToDevice) == hipSuccess)) &&
                         hipMalloc((void**)&d_turned, ndst * 4) == hipSuccess && hipMalloc((void**)&d_sum, sizeof sum) == hipSuccess &&
                         vxrt_transform_stamp(raytracer->Context(), c.d_bits, c.dims, &o, d_turned, d_sum, nullptr) == VXRT_OK &&
                         hipMemcpy(turned.data(), d_turned, ndst * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                         hipMemcpy(&sum, d_sum, sizeof sum, hipMemcpyDeviceToHost) == hipSuccess;
                    (void)hipFree(d_sum);
                    if (ok) {  // the swap: the turned buffer is the slot from here on
                        (void)hipFree(c.d_bits);
                        c.d_bits = d_turned;
                        c.bits.swap(turned);
                        for (int k = 0; k < 3; ++k)
                            c.dims[k] = dd[k];
                    } else {
                        (void)hipFree(d_turned);
                    }
                }
                if (!ok) {
                    std::cerr << what << " before frame " << from << ": "
                              << (it == clipboard.end() ? "empty clipboard slot" : vxrt_last_error()) << std::endl;
                    std::exit(3);
                }
                uint64_t h = 0xcbf29ce484222325ull;
                const std::vector<uint32_t>& bits = it->second.bits;
                for (size_t i = 0; i < bits.size() * 4; ++i)
                    h = (h ^ ((const unsigned char*)bits.data())[i]) * 0x100000001b3ull;
                std::printf("%s before frame %d: slot %d, dims %d %d %d, %llu voxels, box %d %d %d %d %d %d, hash %016llx\n", what, from,
                            e.op.value, dd[0], dd[1], dd[2], (unsigned long long)sum.voxels, sum.set_min[0], sum.set_min[1], sum.set_min[2],
                            sum.set_max[0], sum.set_max[1], sum.set_max[2], (unsigned long long)h);
            } else if (e.op.kind == 3) {  // paste
                flush_ops();
                const auto it = clipboard.find(e.op.value);
                vxrt_edit_stats st{};
                if (it == clipboard.end() || e.op.b[1] != 0 || e.op.b[2] != 0 ||
                    raytracer->StampVoxels(e.op.a, it->second.dims, it->second.bits.data(), e.op.b[0], &st) != VXRT_OK) {
                    std::cerr << "paste before frame " << from << ": " << (it == clipboard.end() ? "empty clipboard slot" : vxrt_last_error())
                              << std::endl;
                    std::exit(3);
                }
                std::printf("paste before frame %d: slot %d, %llu bricks touched, %llu created, %llu freed\n", from, e.op.value,
                            (unsigned long long)st.bricks_touched, (unsigned long long)st.bricks_created, (unsigned long long)st.bricks_freed);
            } else {
                ops.push_back(e.op);
            }
        }
        flush_ops();
    };

    // the camera pose of frame i: the path's (or the fixed camera), then with walk=1 the body moved toward it
    const float half[3] = {2.0f, 6.0f, 2.0f};
    vxrt_body body{};
    bool body_placed = false;
    auto pose_for = [&](int i) {
        if (!path.empty()) {
            cam_pos = path[(size_t)i].pos;
            cam_eular = path[(size_t)i].euler;
        }
        if (!walk)
            return;
        const float target[3] = {cam_pos.x, cam_pos.y, cam_pos.z};
        for (int k = 0; k < 3; ++k) {
            if (!body_placed) {
                body.lo[k] = target[k] - half[k];
                body.hi[k] = target[k] + half[k];
            }
            const float d = target[k] - (body.lo[k] + half[k]);
            const float m = (float)VXRT_BODY_MAX_DELTA;
            body.delta[k] = d > m ? m : (d < -m ? -m : d);
        }
        body_placed = true;
        float lohi[6];
        uint32_t flags = 0;
        if (raytracer->MoveBoxes(&body, 1, lohi, &flags) != VXRT_OK) {
            std::cerr << "walk, frame " << i << ": " << vxrt_last_error() << std::endl;
            std::exit(3);
        }
        for (int k = 0; k < 3; ++k) {
            body.lo[k] = lohi[k];
            body.hi[k] = lohi[3 + k];
        }
        cam_pos = make_float3(body.lo[0] + half[0], body.lo[1] + half[1], body.lo[2] + half[2]);
        std::printf("walk frame %d lo %a %a %a hi %a %a %a flags %u\n", i, body.lo[0], body.lo[1], body.lo[2], body.hi[0],
                    body.hi[1], body.hi[2], flags);
    };

    void* d_pixels = nullptr;
    if (hipMalloc(&d_pixels, (size_t)width * height * sizeof(BGRA8888)) != hipSuccess)
        return 1;
    (void)hipMemset(d_pixels, 255, (size_t)width * height * sizeof(BGRA8888));
    std::vector<BGRA8888> pixels((size_t)width * height);

    auto write_ppm = [&](const std::string& name) {
        std::ofstream ppm(name, std::ios::binary);
        ppm << "P6\n" << width << " " << height << "\n255\n";
        for (const auto& p : pixels) {
            const char rgb[3] = {(char)p.r, (char)p.g, (char)p.b};
            ppm.write(rgb, 3);
        }
    };

    double avgFrameTime = 0.0;
    const int nframes = path.empty() ? frames : (int)path.size();
    // buffers of the two-frames-in-flight mode (allocated before the timed frame loop, like d_pixels)
    void* d_ring[3] = {d_pixels, nullptr, nullptr};
    BGRA8888* h_ring[3] = {nullptr, nullptr, nullptr};
    hipEvent_t rendered[3], copied[3];
    hipStream_t copy_stream;
    const size_t bytes = (size_t)width * height * sizeof(BGRA8888);
    if (hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking) != hipSuccess)
        return 1;
    for (int k = 0; k < 3 && in_flight >= 2 && batch <= 1; ++k) {
        if ((k > 0 && hipMalloc(&d_ring[k], bytes) != hipSuccess) || hipHostMalloc((void**)&h_ring[k], bytes) != hipSuccess ||
            hipEventCreateWithFlags(&rendered[k], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&copied[k], hipEventDisableTiming) != hipSuccess)
            return 1;
        (void)hipMemset(d_ring[k], 255, bytes);
    }
    vxrt_frame_stats rays_before{};
    (void)vxrt_frame_stats_get(raytracer->Context(), &rays_before);  // start the ray counters of the frame loop from zero
    const auto loop0 = std::chrono::high_resolution_clock::now();
    double dump_ms = 0.0;
    auto timed_dump = [&](int i) {
        if (!dump_all)
            return;
        const auto d0 = std::chrono::high_resolution_clock::now();
        char name[32];
        std::snprintf(name, sizeof(name), "_%04d.ppm", i);
        write_ppm(prefix + name);
        dump_ms += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - d0).count() / 1000.0;
    };
    if (batch <= 1 && in_flight >= 2) {
        // Two frames in flight (Graphics::RenderScreenAsync): launch frame i, queue its device->host copy behind it on the
        // frame's stream, THEN take delivery of frame i-2 -- the per-frame sequence of VoxelApp/main.cu:165-167 with the
        // host two frames ahead of the pixels.  The camera of frame i may depend on anything the host knows when it launches
        // it; nothing is batched ahead.  Three device buffers and three pinned host buffers rotate.
        for (int i = 0; i < nframes + 2; ++i) {
            auto f0 = std::chrono::high_resolution_clock::now();
            if (i < nframes) {
                apply_edits(i, i + 1);
                pose_for(i);
                GetDirections(cam_eular, &cam_forward, &cam_up, &cam_right);
                const FrameTicket t = RenderScreenAsync(raytracer, width, height, d_ring[i % 3], cam_pos, cam_forward, cam_up, cam_right);
                // the copy runs on its own stream behind the frame, so the render streams never wait for the copy engine
                (void)hipEventRecord(rendered[i % 3], (hipStream_t)FrameStream(t));
                (void)hipStreamWaitEvent(copy_stream, rendered[i % 3], 0);
                (void)hipMemcpyAsync(h_ring[i % 3], d_ring[i % 3], bytes, hipMemcpyDeviceToHost, copy_stream);
                (void)hipEventRecord(copied[i % 3], copy_stream);
            }
            if (i >= 2) {  // frame i-2 is delivered (its device buffer is the one frame i+1 will render into)
                (void)hipEventSynchronize(copied[(i - 2) % 3]);
                if (dump_all || i - 2 == nframes - 1)
                    std::memcpy(pixels.data(), h_ring[(i - 2) % 3], bytes);
                timed_dump(i - 2);
            }
            auto f1 = std::chrono::high_resolution_clock::now();
            double td = std::chrono::duration_cast<std::chrono::microseconds>(f1 - f0).count() / 1000.0;
            avgFrameTime = i == 0 ? td : avgFrameTime * 0.9 + td * 0.1;
        }
    }
    if (batch > 1) {
        // several poses per launch (Graphics::RenderScreens): every view has its own framebuffer, so this mode runs
        // without the checkerboard's frame-to-frame history
        RenderSwitches s;
        s.DebugView = !shaded;
        s.Checkerboard = false;
        s.ShadowRay = shaded;
        s.BounceSamples = shaded ? 1 : 0;
        SetRenderSwitches(s);
        std::vector<void*> d_views((size_t)batch, nullptr);
        for (auto& p : d_views)
            if (hipMalloc(&p, (size_t)width * height * sizeof(BGRA8888)) != hipSuccess)
                return 1;
        for (int first = 0; first < nframes; first += batch) {
            const int n = nframes - first < batch ? nframes - first : batch;
            std::vector<ScreenView> views((size_t)n);
            apply_edits(first, first + n);
            auto f0 = std::chrono::high_resolution_clock::now();
            for (int j = 0; j < n; ++j) {
                pose_for(first + j);
                GetDirections(cam_eular, &cam_forward, &cam_up, &cam_right);
                views[(size_t)j] = ScreenView{d_views[(size_t)j], cam_pos, cam_forward, cam_up, cam_right};
            }
            RenderScreens(raytracer, width, height, views.data(), (uint32_t)n);
            auto f1 = std::chrono::high_resolution_clock::now();
            double td = std::chrono::duration_cast<std::chrono::microseconds>(f1 - f0).count() / 1000.0 / n;
            avgFrameTime = first == 0 ? td : avgFrameTime * 0.9 + td * 0.1;
            for (int j = 0; j < n; ++j) {
                (void)hipMemcpy(pixels.data(), d_views[(size_t)j], pixels.size() * sizeof(BGRA8888), hipMemcpyDeviceToHost);
                timed_dump(first + j);
            }
        }
        for (auto p : d_views)
            (void)hipFree(p);
    }
    // the frame denoiser's buffers: colour AOV, hit-index AOV, keys, workspace -- allocated once, when the script asks for it
    float* d_color = nullptr;
    int64_t* d_hit = nullptr;
    uint32_t* d_keys_pair[2] = {nullptr, nullptr};  // this frame's keys and the previous frame's, swapped per frame
    void* d_dn_work = nullptr;
    vxrt_history* d_hist[2] = {nullptr, nullptr};
    vxrt_reproject_summary* d_rp_sum = nullptr;
    uint8_t* d_levels = nullptr;
    float* d_lit = nullptr;  // the lit colours: the frame's own colours stay what the next frame's history expects
    vxrt_light_frame_summary* d_lf_sum = nullptr;
    float* d_mat = nullptr;  // the coloured frame: as d_lit, beside the frame's own colours
    vxrt_material* d_palette = nullptr;
    uint32_t* d_atlas = nullptr;
    vxrt_material_frame_summary* d_mat_sum = nullptr;
    float* d_sky = nullptr;  // the finished frame: as d_lit, beside the frame's own colours
    vxrt_sky_summary* d_sky_sum = nullptr;
    if (!denoise_lines.empty() || !temporal_lines.empty() || !lit_lines.empty() || !materials_lines.empty() || !sky_lines.empty()) {
        const size_t n = (size_t)width * height;
        if (batch > 1 || in_flight >= 2 || shade_mode == 1 || vxrt_denoise_workspace_bytes(width, height) == 0) {
            std::cerr << "denoise, temporal, lit, materials, sky: whole frames only (shaded=0 or 2, views_per_launch=1, frames_in_flight=1)" << std::endl;
            return 2;
        }
        if (hipMalloc((void**)&d_color, n * 12) != hipSuccess || hipMalloc((void**)&d_hit, n * 8) != hipSuccess ||
            hipMalloc((void**)&d_keys_pair[0], n * 4) != hipSuccess || hipMalloc((void**)&d_keys_pair[1], n * 4) != hipSuccess ||
            hipMalloc(&d_dn_work, vxrt_denoise_workspace_bytes(width, height)) != hipSuccess)
            return 1;
        if (!temporal_lines.empty() &&
            (hipMalloc((void**)&d_hist[0], n * 16) != hipSuccess || hipMalloc((void**)&d_hist[1], n * 16) != hipSuccess ||
             hipMalloc((void**)&d_rp_sum, sizeof(vxrt_reproject_summary)) != hipSuccess))
            return 1;
        if (!lit_lines.empty() &&
            (hipMalloc((void**)&d_lit, n * 12) != hipSuccess || hipMalloc((void**)&d_lf_sum, sizeof(vxrt_light_frame_summary)) != hipSuccess))
            return 1;
        if (!sky_lines.empty() &&
            (hipMalloc((void**)&d_sky, n * 12) != hipSuccess || hipMalloc((void**)&d_sky_sum, sizeof(vxrt_sky_summary)) != hipSuccess))
            return 1;
        if (!materials_lines.empty()) {
            // grass, dirt, stone, sand, snow (materials 1 .. 5): white tints, tiles 0 .. 4, and tile 5 on the sides of grass
            std::vector<vxrt_material> palette(256);
            for (auto& m : palette) {
                m.tint[0] = m.tint[1] = m.tint[2] = 1.0f;
                m.tile_top = m.tile_side = m.tile_bottom = VXRT_MATERIAL_NO_TILE;
                m.reserved = 0;
            }
            for (uint16_t m = 1; m <= 5; ++m)
                palette[m].tile_top = palette[m].tile_side = palette[m].tile_bottom = (uint16_t)(m - 1);
            palette[1].tile_side = 5;
            palette[1].tile_bottom = 1;  // dirt under a grass block
            const uint32_t base[6][3] = {{80, 180, 60}, {134, 96, 67}, {128, 128, 128}, {220, 205, 140}, {245, 245, 255}, {110, 140, 70}};
            std::vector<uint32_t> atlas(6 * 64);
            for (uint32_t t = 0; t < 6; ++t)
                for (uint32_t r = 0; r < 8; ++r)
                    for (uint32_t s2 = 0; s2 < 8; ++s2) {
                        const uint32_t n = (((t * 73856093u) ^ (r * 19349663u) ^ (s2 * 83492791u)) * 2654435761u) >> 24;
                        const uint32_t shade = 192u + (n >> 2);  // 192 .. 255
                        atlas[(t * 8 + r) * 8 + s2] = (base[t][0] * shade / 255u) | (base[t][1] * shade / 255u) << 8 | (base[t][2] * shade / 255u) << 16 | 0xFF000000u;
                    }
            if (hipMalloc((void**)&d_mat, n * 12) != hipSuccess || hipMalloc((void**)&d_palette, 256 * sizeof(vxrt_material)) != hipSuccess ||
                hipMalloc((void**)&d_atlas, atlas.size() * 4) != hipSuccess || hipMalloc((void**)&d_mat_sum, sizeof(vxrt_material_frame_summary)) != hipSuccess ||
                hipMemcpy(d_palette, palette.data(), 256 * sizeof(vxrt_material), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(d_atlas, atlas.data(), atlas.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
                return 1;
        }
    }
    vxrt_material_rules mat_rules{};
    mat_rules.struct_size = sizeof(vxrt_material_rules);
    mat_rules.n_bands = 2;
    mat_rules.bands[0] = vxrt_material_band{INT32_MIN, 1, 2, 3, 3};              // grass, three of dirt, stone
    mat_rules.bands[1] = vxrt_material_band{(int32_t)((wy ? wy : edge) / 8 * 5), 5, 4, 3, 1};  // snow, one of sand, stone
    mat_rules.paint_dims[0] = mat_rules.paint_dims[1] = mat_rules.paint_dims[2] = 1;
    vxrt_material_frame_params mf{};
    mf.struct_size = sizeof(vxrt_material_frame_params);
    mf.n_tiles = 6;
    mf.tile_shift = 3;
    bool materials = false;
    vxrt_material_frame_summary mat_sum{};
    vxrt_denoise_params dn{sizeof(vxrt_denoise_params), 0, 0.0f, 0};
    vxrt_reproject_params rp{};
    rp.struct_size = sizeof(vxrt_reproject_params);
    bool temporal = false, have_history = false;
    vxrt_reproject_summary rp_sum{};
    vxrt_light_frame_params lf{};
    lf.struct_size = sizeof(vxrt_light_frame_params);
    lf.flags = VXRT_LF_SMOOTH | VXRT_LF_OCCLUSION;
    lf.outside_level = 0xF0u;
    const float lf_block[3] = {1.0f, 0.8f, 0.5f}, lf_curve[4] = {0.4f, 0.6f, 0.8f, 1.0f};
    std::memcpy(lf.block_color, lf_block, sizeof lf_block);
    std::memcpy(lf.ao_curve, lf_curve, sizeof lf_curve);
    bool lit = false;
    vxrt_light_frame_summary lf_sum{};
    // the daytime preset (the defaults of the Python mirror's Sky), its sun in the environment's light direction
    vxrt_sky_params sp{};
    sp.struct_size = sizeof(vxrt_sky_params);
    sp.glow_log2 = 3;
    sp.octaves = 4;
    sp.seed = 1;
    const float sky_colours[5][3] = {{0.18f, 0.38f, 0.80f}, {0.70f, 0.82f, 0.95f}, {0.30f, 0.28f, 0.25f}, {1.0f, 0.95f, 0.80f}, {1.0f, 1.0f, 1.0f}};
    float* const sky_slots[5] = {sp.zenith, sp.horizon, sp.ground, sp.sun_color, sp.cloud_color};
    for (int k = 0; k < 5; ++k)
        std::memcpy(sky_slots[k], sky_colours[k], sizeof sky_colours[k]);
    sp.sun_dir[0] = env.LightDirection.x;
    sp.sun_dir[1] = env.LightDirection.y;
    sp.sun_dir[2] = env.LightDirection.z;
    sp.glow_strength = 0.35f;
    sp.ground_fade = 4.0f;
    sp.cos_inner = 0.9995f;
    sp.cos_outer = 0.9985f;
    sp.cloud_y = 2.0f * (float)(wy ? wy : edge);
    sp.cloud_scale = 0.004f;
    sp.cloud_max_t = 20000.0f;
    sp.cloud_cover = 0.5f;
    sp.cloud_sharp = 3.0f;
    sp.cloud_fade = 6.0f;
    sp.fog_start = 64.0f;
    sp.fog_density = 0.0015f;
    sp.fog_max = 0.85f;
    bool sky = false;
    vxrt_sky_summary sky_sum{};
    for (int i = 0; batch <= 1 && in_flight < 2 && i < nframes; ++i) {
        apply_edits(i, i + 1);
        for (const DenoiseLine& l : denoise_lines)
            if (l.frame == i) {
                dn.iterations = l.iterations;
                dn.color_scale = l.color_scale;
            }
        for (const TemporalLine& l : temporal_lines)
            if (l.frame == i) {
                temporal = l.on;
                rp.max_history = l.max_history;
            }
        for (const MaterialsLine& l : materials_lines)
            if (l.frame == i)
                materials = l.on;
        for (const SkyLine& l : sky_lines)
            if (l.frame == i) {
                sky = l.on;
                sp.flags = l.clouds ? VXRT_SKY_CLOUDS : 0u;
            }
        for (const LitLine& l : lit_lines)
            if (l.frame == i) {
                lit = l.on;
                if (!lit)
                    continue;
                // the box's light field, once: both channels, the line's emitters; the levels stay on the device
                const uint64_t nvox = (uint64_t)(l.dims[0] > 0 ? l.dims[0] : 0) * (uint64_t)(l.dims[1] > 0 ? l.dims[1] : 0) *
                                      (uint64_t)(l.dims[2] > 0 ? l.dims[2] : 0);
                std::vector<uint8_t> levels(nvox > 0 && nvox <= (1ull << 28) ? (size_t)nvox : 1u);
                vxrt_light_summary ls{};
                (void)hipFree(d_levels);
                d_levels = nullptr;
                if (vxrt_light_field_host(raytracer->Context(), l.origin, l.dims, l.emitters.empty() ? nullptr : l.emitters.data(),
                                          (uint32_t)(l.emitters.size() / 4), VXRT_LIGHT_SKY | VXRT_LIGHT_BLOCK, levels.data(), &ls) != VXRT_OK ||
                    hipMalloc((void**)&d_levels, levels.size()) != hipSuccess ||
                    hipMemcpy(d_levels, levels.data(), levels.size(), hipMemcpyHostToDevice) != hipSuccess) {
                    std::cerr << "lit, frame " << i << ": " << vxrt_last_error() << std::endl;
                    return 3;
                }
                for (int k = 0; k < 3; ++k) {
                    lf.box_origin[k] = l.origin[k];
                    lf.box_dims[k] = l.dims[k];
                }
                lf.sky_floor = l.sky_floor;
            }
        for (const EditLine& e : edits)
            if (e.frame == i)
                have_history = false;  // shadows and bounces change far from an edit's box: the history starts anew
        uint32_t* const d_keys = d_keys_pair[i & 1];
        pose_for(i);
        auto f0 = std::chrono::high_resolution_clock::now();
        GetDirections(cam_eular, &cam_forward, &cam_up, &cam_right);
        if (dn.iterations > 0 || temporal || lit || materials || sky) {
            // the frame with its AOVs through the C ABI (the facade's RenderScreen has no AOV arguments), then keys and filter
            vxrt_ctx* c = raytracer->Context();
            const float o[3] = {cam_pos.x, cam_pos.y, cam_pos.z}, f[3] = {cam_forward.x, cam_forward.y, cam_forward.z},
                        u[3] = {cam_up.x, cam_up.y, cam_up.z}, r[3] = {cam_right.x, cam_right.y, cam_right.z};
            const float L[3] = {env.LightDirection.x, env.LightDirection.y, env.LightDirection.z}, C[3] = {2, 2, 2}, A[3] = {0.5f, 0.5f, 0.5f};
            vxrt_render_flags fl;
            vxrt_render_flags_default(&fl);
            fl.mode = shaded ? VXRT_MODE_SHADED : VXRT_MODE_DEBUG;
            fl.shadow = shaded;
            fl.bounce_samples = shaded ? 1 : 0;
            fl.d_color_aov = d_color;
            fl.d_hit_aov = d_hit;
            if (vxrt_set_environment(c, L, C, A) != VXRT_OK || vxrt_set_fov(c, 90) != VXRT_OK || vxrt_set_ortho_window_size(c, 10, 10) != VXRT_OK ||
                vxrt_render(c, width, height, d_pixels, o, f, u, r, &fl) != VXRT_OK ||
                vxrt_frame_guides(c, width, height, o, f, u, r, 0, d_hit, d_keys, nullptr) != VXRT_OK) {
                std::cerr << "render and guides, frame " << i << ": " << vxrt_last_error() << std::endl;
                return 3;
            }
            if (temporal) {
                // the previous frame's history and keys (none at the first such frame and after an edit), its pose in rp.cur
                rp.prev = rp.cur;
                for (int k = 0; k < 3; ++k) {
                    rp.cur.origin[k] = o[k];
                    rp.cur.fwd[k] = f[k];
                    rp.cur.up[k] = u[k];
                    rp.cur.right[k] = r[k];
                }
                if (!have_history)
                    rp.prev = rp.cur;
                if (vxrt_reproject_frame(c, width, height, d_color, d_keys, have_history ? d_hist[(i + 1) & 1] : nullptr,
                                         have_history ? d_keys_pair[(i + 1) & 1] : nullptr, &rp, d_hist[i & 1], d_color, d_pixels, d_rp_sum,
                                         nullptr) != VXRT_OK) {
                    std::cerr << "temporal, frame " << i << ": " << vxrt_last_error() << std::endl;
                    return 3;
                }
            }
            if ((dn.iterations > 0 &&
                 vxrt_denoise_frame(c, width, height, d_color, d_keys, &dn, d_dn_work, d_color, d_pixels, nullptr) != VXRT_OK) ||
                vxrt_synchronize(c) != VXRT_OK) {
                std::cerr << "denoise, frame " << i << ": " << vxrt_last_error() << std::endl;
                return 3;
            }
            if (temporal)
                (void)hipMemcpy(&rp_sum, d_rp_sum, sizeof(rp_sum), hipMemcpyDeviceToHost);
            if (materials) {
                for (int k = 0; k < 3; ++k) {
                    mf.cam.origin[k] = o[k];
                    mf.cam.fwd[k] = f[k];
                    mf.cam.up[k] = u[k];
                    mf.cam.right[k] = r[k];
                }
                if (vxrt_material_frame(c, width, height, d_color, d_keys, d_hit, &mat_rules, nullptr, d_palette, d_atlas, &mf, d_mat, d_pixels,
                                        nullptr, d_mat_sum, nullptr) != VXRT_OK ||
                    vxrt_synchronize(c) != VXRT_OK) {
                    std::cerr << "materials, frame " << i << ": " << vxrt_last_error() << std::endl;
                    return 3;
                }
                (void)hipMemcpy(&mat_sum, d_mat_sum, sizeof(mat_sum), hipMemcpyDeviceToHost);
            }
            if (lit) {
                for (int k = 0; k < 3; ++k) {
                    lf.cam.origin[k] = o[k];
                    lf.cam.fwd[k] = f[k];
                    lf.cam.up[k] = u[k];
                    lf.cam.right[k] = r[k];
                }
                if (vxrt_light_frame(c, width, height, materials ? d_mat : d_color, d_keys, d_hit, d_levels, &lf, d_lit, d_pixels, nullptr, d_lf_sum,
                                     nullptr) !=
                        VXRT_OK ||
                    vxrt_synchronize(c) != VXRT_OK) {
                    std::cerr << "lit, frame " << i << ": " << vxrt_last_error() << std::endl;
                    return 3;
                }
                (void)hipMemcpy(&lf_sum, d_lf_sum, sizeof(lf_sum), hipMemcpyDeviceToHost);
            }
            if (sky) {
                for (int k = 0; k < 3; ++k) {
                    sp.cam.origin[k] = o[k];
                    sp.cam.fwd[k] = f[k];
                    sp.cam.up[k] = u[k];
                    sp.cam.right[k] = r[k];
                }
                if (vxrt_sky_frame(c, width, height, lit ? d_lit : materials ? d_mat : d_color, d_keys, &sp, d_sky, d_pixels, d_sky_sum, nullptr) !=
                        VXRT_OK ||
                    vxrt_synchronize(c) != VXRT_OK) {
                    std::cerr << "sky, frame " << i << ": " << vxrt_last_error() << std::endl;
                    return 3;
                }
                (void)hipMemcpy(&sky_sum, d_sky_sum, sizeof(sky_sum), hipMemcpyDeviceToHost);
            }
        } else {
            RenderScreen(raytracer, width, height, d_pixels, cam_pos, cam_forward, cam_up, cam_right);
        }
        have_history = temporal;
        if (temporal)
            std::printf("temporal frame %d max_history %d hit %u reused %u offscreen %u rejected %u\n", i, rp.max_history, rp_sum.hit,
                        rp_sum.reused, rp_sum.offscreen, rp_sum.rejected);
        if (materials)
            std::printf("materials frame %d hit %u painted %u top %u textured %u\n", i, mat_sum.hit, mat_sum.painted, mat_sum.top, mat_sum.textured);
        if (lit)
            std::printf("lit frame %d hit %u in_box %u occluded %u dark %u\n", i, lf_sum.hit, lf_sum.in_box, lf_sum.occluded, lf_sum.dark);
        if (sky)
            std::printf("sky frame %d miss %u ground %u sun %u cloud %u fogged %u\n", i, sky_sum.miss, sky_sum.ground, sky_sum.sun, sky_sum.cloud,
                        sky_sum.fogged);
        (void)hipMemcpy(pixels.data(), d_pixels, pixels.size() * sizeof(BGRA8888), hipMemcpyDeviceToHost);
        if (dn.iterations > 0) {
            std::vector<uint32_t> keys((size_t)width * height);
            (void)hipMemcpy(keys.data(), d_keys, keys.size() * 4, hipMemcpyDeviceToHost);
            size_t hit = 0;
            std::map<uint32_t, int> faces;
            for (uint32_t k : keys)
                if (k) {
                    ++hit;
                    faces[k] = 1;
                }
            uint64_t h = 0xcbf29ce484222325ull;
            for (size_t b = 0; b < pixels.size() * sizeof(BGRA8888); ++b)
                h = (h ^ ((const unsigned char*)pixels.data())[b]) * 0x100000001b3ull;
            std::printf("denoise frame %d iterations %d color_scale %g hit %zu faces %zu hash %016llx\n", i, dn.iterations,
                        (double)dn.color_scale, hit, faces.size(), (unsigned long long)h);
        }
        auto f1 = std::chrono::high_resolution_clock::now();
        double td = std::chrono::duration_cast<std::chrono::microseconds>(f1 - f0).count() / 1000.0;
        avgFrameTime = i == 0 ? td : avgFrameTime * 0.9 + td * 0.1;
        timed_dump(i);
    }
    std::cout << "Avg FPS: " << 1000.0 / avgFrameTime << std::endl;
    {
        vxrt_frame_stats st{};
        (void)vxrt_frame_stats_get(raytracer->Context(), &st);  // synchronises the device
        const double loop_ms = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - loop0).count() / 1000.0 - dump_ms;
        const unsigned long long rays = st.primary_rays + st.shadow_rays + st.bounce_rays;
        std::printf("Frame loop: %d frames, %llu rays in %.3f ms (device->host copy of every frame included) = %.1f Mrays/s\n", nframes, rays,
                    loop_ms, loop_ms > 0 ? rays / loop_ms / 1e3 : 0.0);
    }

    std::ofstream raw(prefix + ".bgra", std::ios::binary);
    raw.write(reinterpret_cast<const char*>(pixels.data()), (std::streamsize)(pixels.size() * sizeof(BGRA8888)));
    write_ppm(prefix + ".ppm");
    // a few batch queries through VoxelRaytracer3D::Raytrace
    std::vector<float3> o(4, cam_pos), d = {make_float3(0, -1, 0), make_float3(1, -1, 0), make_float3(0, 1, 0), cam_forward};
    auto res = raytracer->Raytrace(o, d);
    for (int i = 0; i < 4; ++i)
        std::printf("ray %d valid=%d steps=%d voxel=%d\n", i, (int)res.valid[i], res.steps[i], res.voxelIndex[i]);
    for (int k = 0; k < 3 && in_flight >= 2 && batch <= 1; ++k) {
        if (k > 0)
            (void)hipFree(d_ring[k]);
        (void)hipHostFree(h_ring[k]);
        (void)hipEventDestroy(rendered[k]);
        (void)hipEventDestroy(copied[k]);
    }
    (void)hipStreamDestroy(copy_stream);
    (void)hipFree(d_color);
    (void)hipFree(d_levels);
    (void)hipFree(d_lit);
    (void)hipFree(d_lf_sum);
    (void)hipFree(d_mat);
    (void)hipFree(d_palette);
    (void)hipFree(d_atlas);
    (void)hipFree(d_mat_sum);
    (void)hipFree(d_sky);
    (void)hipFree(d_sky_sum);
    (void)hipFree(d_hit);
    (void)hipFree(d_keys_pair[0]);
    (void)hipFree(d_keys_pair[1]);
    (void)hipFree(d_hist[0]);
    (void)hipFree(d_hist[1]);
    (void)hipFree(d_rp_sum);
    (void)hipFree(d_dn_work);
    (void)hipFree(d_pixels);
    delete raytracer;
    return 0;
}
