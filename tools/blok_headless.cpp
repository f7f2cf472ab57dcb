// Headless driver shaped like the reference's App (reference blok/src/app.cpp:65-192) with the backend
// switch extended by GraphicsApi::HIP: build a world through ChunkManager, rebuildDirtyChunks,
// packChunksToGpuSvo, addWorld, then a frame loop of drawFrame; writes the last frame as a PPM.
//   blok_headless [--n 256 | --vox model.vox | --obj model.obj [--obj-size 256] [--solid] | --terrain SEED [--terrain-size 256] [--obj model.obj]] [--size 1280x720] [--pose 0|1|2] [--frames 10] [--out frame.ppm] [--rt [--spp 8]] [--export-obj surface.obj] [--components] [--settle] [--save-volume world.bvol] [--seal [--seal-material N]] [--hollow D2] [--rule NB,SURVIVE_HEX,BIRTH_HEX,STEPS[,solid] | --smooth STEPS] [--populate A.vox[,B.vox...] [--bake]] [--scroll DX,DY,DZ] [--stroke X,Y,Z:X,Y,Z:...,R[,OP]] [--lod K[,MIN]] [--far K[,MIN]] [--paste FILE.vox@X,Y,Z,YAW_DEG,SCALE]
//   blok_headless --load-volume world.bvol [--terrain SEED --terrain-size N] ...
//   --obj: a triangle mesh (with its mtllib) fitted into a resident volume of --obj-size^3 voxels and voxelized on the device
//          (surface shell, or filled with --solid), then rebuilt with the library's materials
//   --terrain: procedural terrain generated on the device into a resident volume of --terrain-size^3 voxels (blok_hip_volume_generate_terrain),
//          rebuilt with grass, soil, rock and an emissive ore; the camera stands on blok_terrain_height.  With --obj the mesh is voxelized on
//          top of it, a quarter of the box tall, standing on the ground at the box centre
//   --scroll DX,DY,DZ: with --terrain, after the fill: the box is moved through the world by that many voxels (multiples of 4,
//          blok_hip_volume_scroll), the same terrain is generated into each box that came into view, and the camera moves with the box:
//          the frame shows the terrain as a box generated whole at the new place would.
//   --lod K[,MIN]: with --terrain, once the terrain's world is built: the whole box is reduced K times (1 .. 5) on the device
//          (blok_hip_volume_reduce with BLOK_LOD_VOTE_EXPOSED), level K alone is downloaded — 8^K times fewer cells than the volume — the
//          volume is released, and the coarse cells that hold at least MIN (default 1) filled voxels are installed as the world at voxel
//          size 2^K (blok_hip_set_voxel_size + blok_hip_upload_dense), cell C covering world [C 2^K, (C + 1) 2^K): the frames show the far-field
//          copy of the terrain from the unchanged camera.
//   --far K[,MIN]: with --terrain: the fine box is traced as the world and the eight boxes around it in x and z (the same y range) appear
//          as level-K copies (K in 1 .. 5) at their true size.  Before the terrain's own box is made, the resident volume is created at
//          each neighbour's place in turn, the same terrain generated into it, reduced K times (BLOK_LOD_VOTE_EXPOSED), the cells with at
//          least MIN (default 1) filled voxels taken as a model (blok_hip_volume_lod_model) and the model given the scale 2^K
//          (blok_hip_model_set_scale).  The models become an instance table with identity orientation and offset = the level's first cell
//          times 2^K, traced by blok_hip_trace_primary_instanced (--rt: by the instanced ray-tracing frame).  Prints per neighbour
//          "far: box (x,y,z): N voxels at level K" (a neighbour without such a cell is left out, with 0) and, after the last frame, "far:
//          instances won P of W pixels".  Not with --load-volume, --scroll, --lod, --populate or --obj.
//   --far K[,MIN] --far-direct: the same eight neighbours, the same lines and the same image, through blok_hip_terrain_reduce: the ring is
//          built after the fine box stands, and no volume is made for it.
//   --far K[,MIN] --far-rings R: R rings (1 .. 3; implies --far-direct): ring r is the 8 r boxes of edge --terrain-size at Chebyshev
//          distance r in x and z, reduced to level min(K + r - 1, 5) with MIN clamped to 8^level and placed at that scale; the same line
//          per box, in z-then-x order, ring by ring.
//   --stroke X,Y,Z:X,Y,Z:...,R[,OP]: with --terrain, --obj or --load-volume, before the rebuild: a brush of radius R dragged through the world
//          points (voxels; multiples of one half: W.5 is the centre of voxel W), as one table of capsules in one pass
//          (blok_hip_volume_apply_shapes); OP is add (the default, density 1), subtract (density 0), erase, set, keep or paint (the last
//          three with material 1); prints the number of writes
//   --export-obj: with --terrain or --obj, the resident volume's surface as merged quads (blok_hip_volume_extract_quads over the whole box),
//          written as an OBJ with a sibling .mtl of the library's albedos (blok_quads_write_obj)
//   --components: with --terrain or --obj, the connected components of the whole box (blok_hip_volume_label_components): how many there
//          are, the largest, and how many do not touch the box's floor (floating pieces)
//   --settle: with --terrain or --obj, after --components' pass: every component that does not touch the box's floor is lifted out
//          (blok_hip_volume_capture_component with CUT), swept down against what remains (blok_hip_volume_sweep_models, the box's walls
//          and floor solid) and stamped where it comes to rest (blok_hip_volume_stamp_models); lowest pieces first, pass after pass until
//          nothing floats (at most 8 passes).  The frames show the settled world
//   --save-volume: with --terrain or --obj, after the volume is made and settled: the whole box encoded on the device as a sparse brick
//          stream (blok_hip_volume_encode_bricks), downloaded and written as a .bvol file (blok_bricks_write_file)
//   --load-volume: instead of generating or voxelizing: the file is read and validated (blok_bricks_read_file), a volume of the stream's
//          box created, the stream decoded into it (blok_hip_volume_decode_bricks) and rebuilt with the terrain's four materials.  A file
//          holds voxels, no view: with --terrain SEED --terrain-size N nothing is generated, but the camera stands where that terrain's
//          run puts it, so the frames of a loaded world equal the frames of the run that saved it; without, it looks at the box as --obj's does
//   --hollow D2: with --terrain, --obj or --load-volume, once the volume is filled and before it is rebuilt: the to-empty distance field of the
//          whole box with R = ceil(sqrt(D2)) (blok_hip_volume_distance_field), then BLOK_DISTANCE_HOLLOW at D2: only the shell within D2
//          (a squared distance) of empty space stays.  D2 >= 3 keeps every cell a primary ray can enter, so the frames do not change
//   --rule NB,SURVIVE_HEX,BIRTH_HEX,STEPS[,solid]: with --terrain, --obj or --load-volume, once the volume is filled (and hollowed) and before
//          it is rebuilt: a neighbour-count rule stepped over the whole box (blok_hip_volume_automaton): neighbourhood NB (6, 18, 26), the bit
//          sets of the counts at which a filled cell stays and an empty one is born, in hexadecimal, at most STEPS steps, with "solid" the
//          outside of the box filled; born cells get density 1 and the most frequent id among their filled neighbours.  Prints the info line
//   --smooth STEPS: shorthand for --rule 26,7FFE000,7FFC000,STEPS: the majority of the 26 neighbours (survive at 13 or more, born at 14 or more)
//   --seal: with --terrain, --obj or --load-volume, once the volume is filled and before it is rebuilt: the empty cells of the whole box are
//          flooded from all six faces with max_steps 65534 (blok_hip_volume_flood_field), then BLOK_FLOOD_FILL_UNREACHED fills every empty
//          cell the air did not reach with material 0, or --seal-material N: an openly voxelized shell becomes solid, caves no one can
//          enter are closed.  No primary ray enters a sealed cell
//   --model-lights: with --rt and --populate (without --bake): behind the last rebuild the light table of every loaded model is built from its
//          own tree (blok_hip_model_lights) and the frames go through the instanced path-traced chain (blok_hip_draw_frame_rt_instanced) with the
//          scattered table, so that a model whose material glows (--glow ID) lights the terrain around every copy of it; logs "model lights: M
//          models, F faces; I instances, L lit, A faces in the world" and the camera of the written frame.  Refused when nothing is placed.
//   --populate: with --terrain, once the volume is filled and before it is rebuilt: the first model of every listed .vox file is uploaded
//          (blok_hip_model_create; VOX z is up), the column field of the whole box taken along +y from the top (blok_hip_volume_column_field)
//          and the models scattered on the terrain's grass (blok_hip_volume_scatter_models: seed = the terrain's, one candidate per 16 x 16
//          columns, probability 40000 / 65536, ROTATE | MIRROR, footprint radius 1 with rise and drop of at most 1, each model anchored at
//          the centre of its base).  The first-hit frames are traced with the table as instances (--rt frames show the world alone, unless --model-lights); with
//          --bake the table is stamped into the volume instead (BLOK_STAMP_SET) and the frames show the rebuilt world
//   --paste FILE.vox@X,Y,Z,YAW_DEG,SCALE: with --terrain, once the volume is filled and before it is rebuilt: the first model of the .vox file
//          (VOX z is up) is turned by YAW_DEG about +y around the centre of its voxels' box, scaled by SCALE, and resampled into the volume
//          with that centre at the world point X,Y,Z (blok_affine_from_matrix, blok_hip_volume_stamp_affine, BLOK_STAMP_SET); the number of
//          voxels written is printed.  May be given more than once: pasted in order
//   --pose FILE.vox@X,Y,Z,YAW_DEG[,SCALE]: the first model of the .vox file (VOX z is up) is uploaded and TRACED as a posed model
//          (blok_pose_from_matrix, blok_hip_trace_primary_posed): turned by YAW_DEG about +y around the centre of its voxels' box, scaled by SCALE
//          (1 if left out), that centre at the world point X,Y,Z — --paste's map, shown and not baked.  Over the generated scene (whose material
//          table is the scene's own 256 entries) a voxel's material id is its palette index; with --terrain the palette is imported as materials.
//          The first-hit frames are traced with the poses in the order given; the last frame's camera and `pose: poses won P of W pixels` are
//          printed.  May be given more than once.  Refused with --rt (the path-traced frame takes no pose table), --far, --vox, --obj,
//          --load-volume and more than one device.  (--pose N with a bare number is the camera pose.)
//   --rt: every frame goes through the reference's full ray-tracing path (path trace, denoise, TAA, tonemap, sharpen)
//   --lights: with --rt or --rt-posed over a resident volume (--terrain, --obj, --load-volume): behind the last rebuild the whole box is extracted
//          as quads and the emissive ones become the light table (blok_hip_lights_from_quads) that every path-traced frame samples; logs
//          "lights: N rectangles, A faces, M materials".  --glow ID[:R,G,B] makes material ID of the table the rebuilds install emissive
//          (four times its albedo without R,G,B): --terrain SEED --glow 3 --rt --lights shows lit ore in caves.
//   --light-grid C[,R[,SHARE]]: with --lights: behind the table the light grid is built over it (blok_hip_build_light_grid: cells of 2^C voxels,
//          reach R cells, default 1; the local strategy's share in 1/256, default 192); logs "light grid: N cells (...), M with a list, K items,
//          the longest list L" and the written frame's camera.  Every path-traced frame then samples its lights through the grid.  Refused without --lights.
//   --rt-posed: --rt's chain with the --pose models in it (blok_hip_draw_frame_rt_posed): they cast and receive shadows and show in bounce rays,
//          with their faces' true normals.  Needs at least one --pose FILE.vox@...; prints the written frame's camera as --pose does.  Refused
//          without a --pose and with what --pose refuses.
//   --pose-motion [--pose-spin DEG]: with --rt-posed, the frames are drawn with object motion for the poses (blok_hip_draw_frame_rt_posed_motion),
//          and before drawn frame F (the timed frames 0 .. frames - 1, then the written one) every --pose model is turned to YAW_DEG + F * DEG
//          about its pivot (DEG defaults to 0: the poses rest); `pose: frame F camera ...` is printed for every drawn frame.  Refused without
//          --rt-posed.  Without --pose-motion nothing changes.
//   --devices 0,1,2,...: the frame is tile-partitioned over these devices of the node by ONE process (blok::HipMultiTracer:
//                        RCCL send / receive group or peer copies to the first device); an ordinal may repeat (rehearsal on one GPU)
//   --no-rccl: peer copies even when RCCL is there
//   --dense-exchange: whole RGBA8 tiles travel (RCCL / peer copies) instead of the root reading the ranks' sparse code records
#include <algorithm>
#include <array>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>

#include "blok/hip_tracer.hpp"

namespace {

struct Options {
    uint32_t n = 256, width = 1280, height = 720, frames = 10;     // reference window: 1280x720, app.cpp:95
    int pose = 0;
    std::string out = "frame.ppm";
    bool rt = false;                      // full ray-tracing path per frame instead of first-hit frames
    uint32_t spp = 8;                     // samples per pixel and frame in --rt mode (the reference forces 8)
    std::string vox;                      // optional .vox model instead of the synthetic scene (app.cpp:105-113)
    std::string obj;                      // optional .obj mesh, voxelized into a resident volume
    uint32_t obj_size = 256;
    bool solid = false;
    bool terrain = false;                 // procedural terrain generated on the device
    uint32_t terrain_seed = 0, terrain_size = 256;
    std::string export_obj;               // write the resident volume's surface here
    bool components = false;              // label the resident volume's connected components and print their counts
    bool settle = false;                  // let the components that do not touch the floor fall
    bool seal = false;                    // fill the empty cells that air from the box's faces does not reach, before the rebuild
    uint32_t seal_material = 0;
    int64_t hollow = -1;                  // >= 0: hollow the resident volume at this squared distance before the rebuild
    blok_automaton_rule rule = {};        // steps > 0: step this neighbour-count rule over the resident volume before the rebuild
    bool scroll = false;                  // move the terrain's box by scroll_delta after the fill
    uint32_t lod = 0, lod_min = 1;        // > 0: render level `lod` of the terrain's pyramid, the cells with at least lod_min filled voxels
    bool far_direct = false;              // --far-direct: the ring through blok_hip_terrain_reduce, after the fine box, with no volume of its own
    uint32_t far_rings = 0;               // --far-rings R: R rings (1 .. 3), ring r at level min(far + r - 1, 5); implies far_direct
    uint32_t far = 0, far_min = 1;        // > 0: the eight boxes around the terrain's as level-`far` copies, instances of scaled models
    std::vector<std::array<int32_t, 3>> stroke;      // the points of --stroke, half-voxel units
    uint32_t stroke_radius = 0, stroke_op = BLOK_SHAPE_ADD;
    int32_t scroll_delta[3] = {0, 0, 0};
    std::vector<std::string> populate;    // .vox files whose first models are scattered over the terrain
    bool bake = false;                    // ... and stamped into the volume instead of traced as instances
    struct Paste { std::string path; double position[3], yaw_deg, scale; };
    std::vector<Paste> paste;             // .vox models resampled into the terrain, turned and scaled
    std::vector<Paste> posed;             // .vox models traced as posed models over the world, turned and scaled
    bool rt_posed = false;                // --rt-posed: the ray-tracing path with the posed models in it
    bool lights = false;                  // --lights: with --rt or --rt-posed over a resident volume, its emissive faces are sampled as lights
    bool has_light_grid = false;          // --light-grid C[,R[,SHARE]]: with --lights, the light grid is built over the table (cell_log2, reach, share)
    uint32_t light_grid[3] = {4u, 1u, 192u};
    bool model_lights = false;            // --model-lights: with --rt and --populate, the scattered models' emissive faces are sampled as lights
    struct Glow { uint32_t id; bool has_rgb; float rgb[3]; };
    std::vector<Glow> glow;               // --glow ID[:R,G,B]: materials made emissive in the table every rebuild installs
    bool pose_motion = false;             // --pose-motion: ... drawn with object motion for the poses
    double pose_spin = 0.0;               // --pose-spin DEG: every pose yaws by DEG per drawn frame
    std::string save_volume, load_volume; // the resident volume as a .bvol file, written after it is made / read in place of making it
    std::vector<int> devices;             // more than one entry: the multi-device tracer
    bool dense_exchange = false;
    bool rccl = true;
};

class App {
public:
    App(blok::GraphicsApi api, Options opt) : m_backend(api), m_opt(std::move(opt)), m_mgr(128, 1.0f) {}   // app.cpp:37

    void run() { init(); update(); shutdown(); }                                           // app.cpp:65-71

private:
    void init() {
        switch (m_backend) {
            case blok::GraphicsApi::HIP: {
                m_tracer = std::make_unique<blok::HipTracer>(m_opt.width, m_opt.height);
                m_tracer->init();
                if (!m_opt.posed.empty() && (m_opt.far || !m_opt.vox.empty() || !m_opt.obj.empty() || !m_opt.load_volume.empty() || m_opt.devices.size() > 1))
                    throw std::runtime_error("--pose FILE.vox@... traces its models over the generated scene or a --terrain, on one device: leave --far, --vox, --obj, --load-volume and --devices out");
                if (!m_opt.load_volume.empty() && m_opt.far) throw std::runtime_error("--far generates its terrain: leave --load-volume out");
                if (!m_opt.load_volume.empty() && !m_opt.paste.empty()) throw std::runtime_error("--paste needs a terrain: leave --load-volume out");
                if (!m_opt.load_volume.empty()) { initLoaded(); exportObj(); components(); settle(); saveVolume(); break; }
                if (m_opt.terrain) { initTerrain(); exportObj(); components(); settle(); saveVolume(); lod(); break; }
                if (m_opt.lod) throw std::runtime_error("--lod needs a terrain: --terrain");
                if (m_opt.far) throw std::runtime_error("--far needs a terrain: --terrain");
                if (!m_opt.obj.empty()) { initObj(); exportObj(); components(); settle(); saveVolume(); break; }
                if (!m_opt.export_obj.empty()) throw std::runtime_error("--export-obj needs a resident volume: --terrain or --obj");
                if (m_opt.components) throw std::runtime_error("--components needs a resident volume: --terrain or --obj");
                if (m_opt.settle) throw std::runtime_error("--settle needs a resident volume: --terrain or --obj");
                if (!m_opt.save_volume.empty()) throw std::runtime_error("--save-volume needs a resident volume: --terrain, --obj or --load-volume");
                if (m_opt.hollow >= 0) throw std::runtime_error("--hollow needs a resident volume: --terrain, --obj or --load-volume");
                if (m_opt.rule.steps) throw std::runtime_error("--rule and --smooth need a resident volume: --terrain, --obj or --load-volume");
                if (m_opt.seal) throw std::runtime_error("--seal needs a resident volume: --terrain, --obj or --load-volume");
                if (!m_opt.populate.empty()) throw std::runtime_error("--populate needs a terrain: --terrain");
                if (!m_opt.paste.empty()) throw std::runtime_error("--paste needs a terrain: --terrain");
                if (m_opt.scroll) throw std::runtime_error("--scroll needs a terrain: --terrain");
                if (!m_opt.stroke.empty()) throw std::runtime_error("--stroke needs a resident volume: --terrain, --obj or --load-volume");
                if (!m_opt.vox.empty()) {
                    std::string err;
                    if (!blok::loadAndImportVox(m_opt.vox, m_mgr, &m_materials, nullptr, 0, &err))   // app.cpp:105-113
                        throw std::runtime_error("Failed to load VOX: " + err);
                    m_opt.n = 128;
                } else {
                    uint64_t writes = 0;
                    if (blok_scene_generate(m_mgr.handle(), m_opt.n, 0xB10C0001u, &writes) != BLOK_OK)
                        throw std::runtime_error("scene generation failed (n must be a power of two in [16, 4096])");
                }
                rebuildDirtyChunks(m_mgr, 1 << 30);                                       // app.cpp:120
                packChunksToGpuSvo(m_mgr, m_world);                                       // app.cpp:121
                if (!m_opt.vox.empty()) m_world.materials = m_materials.packForGpu();
                else {
                    m_world.materials.resize(256);
                    blok_scene_materials(0xB10C0001u, m_world.materials.data());
                }
                m_tracer->addWorld(m_world);                                              // app.cpp:122-124
                loadPoses(false);
                if (m_opt.devices.size() > 1) {
                    m_multi = std::make_unique<blok::HipMultiTracer>(m_opt.devices, m_opt.width, m_opt.height, 32, m_opt.rccl);
                    m_multi->addWorld(m_world);
                    if (m_opt.dense_exchange) m_multi->setExchange(0);
                    std::cout << "multi-device: " << m_multi->deviceCount() << " ranks, exchange " << m_multi->exchange() << ", transport " << m_multi->transport() << "\n";
                }
                const blok_world_stats s = m_tracer->worldStats();
                std::cout << "world: " << s.n_voxels << " voxels, " << s.n_ref_nodes << " SVO nodes, " << s.n_sub_chunks
                          << " sub-chunks -> " << s.n_tree_nodes << " tree nodes (" << s.tree_bytes / 1e6 << " MB), "
                          << s.levels << " levels\n";
                blok_camera c{};
                blok_scene_camera(m_opt.n, 0xB10C0001u, m_opt.pose, m_opt.width, m_opt.height, &c);
                for (int a = 0; a < 3; ++a) m_camera.position[a] = c.pos[a];
                m_camera.pitch = std::asin(c.fwd[1]) * 57.29577951308232f;
                m_camera.yaw = std::atan2(c.fwd[2], c.fwd[0]) * 57.29577951308232f;
                break;
            }
            default:
                throw std::runtime_error("this driver only carries the HIP backend");
        }
    }
    // The terrain's parameters for an N^3 box with its four materials registered: grass, soil, rock and an emissive ore.
    blok_terrain_params terrainParams(uint32_t N) {
        blok_terrain_params p{};
        if (blok_terrain_default_params(N, m_opt.terrain_seed, &p) != BLOK_OK) throw std::runtime_error("--terrain-size must be in 1..65536");
        const struct { const char* name; float rgb[3]; float emission; } table[4] = {
            {"grass", {0.25f, 0.62f, 0.20f}, 0.0f}, {"soil", {0.45f, 0.30f, 0.16f}, 0.0f}, {"rock", {0.50f, 0.50f, 0.52f}, 0.0f}, {"ore", {1.0f, 0.55f, 0.10f}, 4.0f}};
        uint32_t ids[4];
        for (int k = 0; k < 4; ++k) {
            blok_material_desc m;
            blok_material_desc_init(&m);
            for (int a = 0; a < 3; ++a) m.albedo[a] = table[k].rgb[a];
            if (table[k].emission > 0.0f) { for (int a = 0; a < 3; ++a) m.emission[a] = table[k].rgb[a]; m.emission_power = table[k].emission; m.type = 3; }
            std::snprintf(m.name, sizeof(m.name), "%s", table[k].name);
            ids[k] = m_materials.addMaterial(m);
        }
        p.surface_material = ids[0]; p.soil_material = ids[1]; p.rock_material = ids[2]; p.ore_material = ids[3];
        return p;
    }
    // The terrain's camera: a few voxels above the highest possible surface over a corner column, looking at a point a little above the ground at the box centre (sky in the upper part of the frame)
    void terrainCamera(const blok_terrain_params& p, uint32_t N, int32_t ground) {
        const float eye[3] = {0.12f * N, static_cast<float>(p.base_height + static_cast<int32_t>(p.amplitude)) + 0.08f * N, 0.10f * N};
        float f[3] = {N / 2.0f - eye[0], static_cast<float>(ground) + 0.15f * N - eye[1], N / 2.0f - eye[2]};
        const float len = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
        const int32_t* at = m_opt.scroll_delta;                  // the box's corner: the camera stands in the box wherever it has gone
        for (int a = 0; a < 3; ++a) { f[a] /= len; m_camera.position[a] = eye[a] + static_cast<float>(a == 1 ? 0 : at[a]); }
        m_camera.pitch = std::asin(f[1]) * 57.29577951308232f;
        m_camera.yaw = std::atan2(f[2], f[0]) * 57.29577951308232f;
    }
    // Terrain generated into an N^3 volume, an optional mesh voxelized on top of it, the camera on the ground near a corner.
    void initTerrain() {
        if (m_opt.devices.size() > 1) throw std::runtime_error("--terrain renders on one device");
        const uint32_t N = m_opt.terrain_size;
        const blok_terrain_params p = terrainParams(N);
        farField(p);
        const int32_t origin[3] = {0, 0, 0};
        m_tracer->createVolume(origin, N, N, N);
        const uint64_t filled = m_tracer->generateTerrain(p);
        std::cout << "terrain: seed " << m_opt.terrain_seed << ", " << N << "^3 -> " << filled << " voxels filled\n";
        if (m_opt.scroll) {
            const blok_scroll_info info = m_tracer->volumeScroll(m_opt.scroll_delta);
            uint64_t generated = 0;
            for (uint32_t b = 0; b < info.n_exposed; ++b) generated += m_tracer->generateTerrain(p, info.exposed[b].lo, info.exposed[b].hi);
            std::cout << "scroll: origin " << info.origin[0] << " " << info.origin[1] << " " << info.origin[2] << ", kept " << info.n_cells_kept << " cells, lost "
                      << info.n_filled_before - info.n_filled_kept << " filled voxels, exposed " << info.n_exposed << " boxes, generated " << generated << " voxels\n";
        }
        const int32_t centre[2] = {static_cast<int32_t>(N / 2) + m_opt.scroll_delta[0], static_cast<int32_t>(N / 2) + m_opt.scroll_delta[2]};
        int32_t ground = 0;
        blok_terrain_height(&p, centre, 1, &ground);
        if (!m_opt.obj.empty()) {
            if (m_opt.scroll) throw std::runtime_error("--scroll does not move a mesh: leave --obj out");
            char err[512] = {0};
            blok_mesh* mesh = nullptr;
            if (blok_obj_load_file(m_opt.obj.c_str(), m_materials.handle(), &mesh, err, sizeof(err)) != BLOK_OK)
                throw std::runtime_error(std::string("Failed to load OBJ: ") + err);
            const size_t nv = blok_mesh_vertex_count(mesh), nt = blok_mesh_triangle_count(mesh);
            std::vector<float> pos(blok_mesh_positions(mesh), blok_mesh_positions(mesh) + 3 * nv);
            std::vector<uint32_t> tri(blok_mesh_triangles(mesh), blok_mesh_triangles(mesh) + 3 * nt);
            std::vector<uint32_t> mat(blok_mesh_materials(mesh), blok_mesh_materials(mesh) + nt);
            blok_mesh_free(mesh);
            if (nt == 0) throw std::runtime_error("the OBJ has no faces");
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            for (size_t i = 0; i < nv; ++i)
                for (int a = 0; a < 3; ++a) { lo[a] = std::min<double>(lo[a], pos[3 * i + a]); hi[a] = std::max<double>(hi[a], pos[3 * i + a]); }
            const double extent = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
            const double scale = extent > 0 ? (N / 4.0) / extent : 1.0;
            for (size_t i = 0; i < nv; ++i) {                    // x, z centred on the box centre; the lowest vertex on top of the ground voxel
                pos[3 * i + 0] = static_cast<float>((pos[3 * i + 0] - (lo[0] + hi[0]) / 2.0) * scale + N / 2.0);
                pos[3 * i + 1] = static_cast<float>((pos[3 * i + 1] - lo[1]) * scale + ground + 1.25);
                pos[3 * i + 2] = static_cast<float>((pos[3 * i + 2] - (lo[2] + hi[2]) / 2.0) * scale + N / 2.0);
            }
            const uint64_t written = m_tracer->voxelizeMesh(pos, tri, mat, 1, 1.0f, m_opt.solid);
            std::cout << "mesh: " << nv << " vertices, " << nt << " triangles -> " << written << " voxels written on the ground at y = " << ground << "\n";
        }
        seal();
        hollow();
        automaton();
        stroke();
        populate(p);
        paste();
        loadPoses(true);
        m_tracer->rebuildVolume(gpuMaterials());
        const blok_world_stats s = m_tracer->worldStats();
        std::cout << "world: " << s.n_voxels << " voxels, " << s.n_tree_nodes << " tree nodes, " << s.levels << " levels\n";
        farFieldDirect(p);
        terrainCamera(p, N, ground);
    }
    // The far field: each of the eight boxes around the terrain's in x and z, generated where it lies, reduced, and kept as a scaled model.
    void farField(const blok_terrain_params& p) {
        if (!m_opt.far) return;
        if (m_opt.scroll || m_opt.lod || !m_opt.populate.empty() || !m_opt.obj.empty())
            throw std::runtime_error("--far shows the terrain and its ring alone: leave --scroll, --lod, --populate, --obj and --load-volume out");
        if (!m_opt.paste.empty()) throw std::runtime_error("--far shows the terrain and its ring alone: leave --paste out");
        if (m_opt.far_direct) return;                           // (farFieldDirect, once the fine box stands)
        const uint32_t N = m_opt.terrain_size, K = m_opt.far;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!dx && !dz) continue;
                const int32_t origin[3] = {dx * static_cast<int32_t>(N), 0, dz * static_cast<int32_t>(N)};
                m_tracer->createVolume(origin, N, N, N);
                m_tracer->generateTerrain(p);
                farPlace(origin, m_tracer->reduceVolume(nullptr, nullptr, K, BLOK_LOD_VOTE_EXPOSED), K, m_opt.far_min);
            }
        farCheck();
    }
    // --far-direct, --far-rings: the same boxes through blok_hip_terrain_reduce, with the fine box in place and no volume made for them;
    // ring r (the 8 r boxes at Chebyshev distance r in x and z) at level min(K + r - 1, 5).
    void farFieldDirect(const blok_terrain_params& p) {
        if (!m_opt.far || !m_opt.far_direct) return;
        const int32_t N = static_cast<int32_t>(m_opt.terrain_size);
        for (int r = 1; r <= static_cast<int>(std::max(m_opt.far_rings, 1u)); ++r) {
            const uint32_t level = std::min<uint32_t>(m_opt.far + static_cast<uint32_t>(r) - 1u, BLOK_LOD_MAX_LEVELS);
            for (int dz = -r; dz <= r; ++dz)
                for (int dx = -r; dx <= r; ++dx) {
                    if (std::max(std::abs(dx), std::abs(dz)) != r) continue;
                    const int32_t origin[3] = {dx * N, 0, dz * N}, end[3] = {origin[0] + N, N, origin[2] + N};
                    farPlace(origin, m_tracer->reduceTerrain(p, origin, end, level, BLOK_LOD_VOTE_EXPOSED), level, std::min(m_opt.far_min, 1u << (3u * level)));
                }
        }
        farCheck();
    }
    // Level `level` of the snapshot just taken of the box at `origin`: its cells with at least minCount voxels as a model of scale 2^level, placed.
    void farPlace(const int32_t origin[3], const blok_lod_info& info, uint32_t level, uint32_t minCount) {
        const blok_lod_level& L = info.level[level - 1];
        uint32_t model = 0;
        uint64_t voxels = 0;
        const int rc = blok_hip_volume_lod_model(m_tracer->handle(), level, minCount, &model, &voxels);
        if (rc != BLOK_OK && rc != BLOK_ERR_UNSUPPORTED) throw std::runtime_error(std::string("HipTracer: ") + blok_hip_last_error(m_tracer->handle()));
        if (rc == BLOK_ERR_UNSUPPORTED) voxels = 0;     // no cell holds that many voxels: the neighbour is left out
        std::cout << "far: box (" << origin[0] << "," << origin[1] << "," << origin[2] << "): " << voxels << " voxels at level " << level << "\n";
        if (!voxels) return;
        m_tracer->setModelScale(model, level);
        blok_instance I{};
        I.model = model;
        for (int a = 0; a < 3; ++a) { I.offset[a] = L.clo[a] * (1 << level); I.axis[a] = static_cast<uint8_t>(a); }
        m_instances.push_back(I);
    }
    void farCheck() {
        if (blok_hip_check_instances(m_tracer->handle(), m_instances.data(), static_cast<uint32_t>(m_instances.size())) != BLOK_OK)
            throw std::runtime_error(std::string("--far: ") + blok_hip_last_error(m_tracer->handle()));
    }
    // After the last frame: how many pixels of the first-hit frame the far field's instances win.
    void farReport() {
        if (!m_opt.far) return;
        const blok_camera c = m_camera.basis(m_opt.width, m_opt.height);
        std::vector<uint32_t> ids(static_cast<size_t>(m_opt.width) * m_opt.height);
        if (blok_hip_trace_primary_instanced(m_tracer->handle(), &c, 0, 0, m_opt.width, m_opt.height, m_instances.data(), static_cast<uint32_t>(m_instances.size()),
                                             nullptr, nullptr, ids.data()) != BLOK_OK)
            throw std::runtime_error(std::string("HipTracer: ") + blok_hip_last_error(m_tracer->handle()));
        size_t won = 0;
        for (uint32_t id : ids) won += id != BLOK_INSTANCE_NONE;
        std::cout << "far: instances won " << won << " of " << ids.size() << " pixels\n";
    }
    // A world read from a .bvol file in place of generating one: a volume of the stream's box, the stream decoded into it, rebuilt.
    void initLoaded() {
        if (m_opt.devices.size() > 1) throw std::runtime_error("--load-volume renders on one device");
        if (!m_opt.obj.empty()) throw std::runtime_error("--load-volume takes the place of --obj");
        char err[512] = {0};
        blok::HipTracer::BrickStream s;
        if (blok_bricks_read_file(m_opt.load_volume.c_str(), &s.info, nullptr, nullptr, nullptr, err, sizeof(err)) != BLOK_OK)
            throw std::runtime_error(std::string("Failed to load volume: ") + err);
        s.records.resize(s.info.n_bricks); s.density.resize(s.info.n_density); s.material.resize(s.info.n_material);
        if (blok_bricks_read_file(m_opt.load_volume.c_str(), &s.info, s.records.data(), s.density.data(), s.material.data(), err, sizeof(err)) != BLOK_OK)
            throw std::runtime_error(std::string("Failed to load volume: ") + err);
        const uint32_t* ext = s.info.ext;
        if (!ext[0] || !ext[1] || !ext[2]) throw std::runtime_error("Failed to load volume: the stream's box is empty");
        const uint32_t N = m_opt.terrain ? m_opt.terrain_size : std::max(ext[0], std::max(ext[1], ext[2]));
        const blok_terrain_params p = terrainParams(N);
        m_tracer->createVolume(s.info.lo, ext[0], ext[1], ext[2]);
        m_tracer->decodeBricks(s);
        seal();
        hollow();
        automaton();
        stroke();
        m_tracer->rebuildVolume(gpuMaterials());
        const blok_world_stats w = m_tracer->worldStats();
        std::cout << "volume loaded: " << s.info.n_bricks << " bricks, " << s.info.n_voxels << " voxels; world: " << w.n_voxels << " voxels, " << w.n_tree_nodes
                  << " tree nodes, " << w.levels << " levels\n";
        if (m_opt.terrain) {
            const int32_t centre[2] = {static_cast<int32_t>(N / 2), static_cast<int32_t>(N / 2)};
            int32_t ground = 0;
            blok_terrain_height(&p, centre, 1, &ground);
            terrainCamera(p, N, ground);
            return;
        }
        const float n = static_cast<float>(N);
        const float eye[3] = {s.info.lo[0] - 0.35f * n, s.info.lo[1] + 1.15f * n, s.info.lo[2] - 0.45f * n};
        float f[3] = {s.info.lo[0] + ext[0] / 2.0f - eye[0], s.info.lo[1] + ext[1] / 2.0f - eye[1], s.info.lo[2] + ext[2] / 2.0f - eye[2]};
        const float len = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
        for (int a = 0; a < 3; ++a) { f[a] /= len; m_camera.position[a] = eye[a]; }
        m_camera.pitch = std::asin(f[1]) * 57.29577951308232f;
        m_camera.yaw = std::atan2(f[2], f[0]) * 57.29577951308232f;
    }
    // Every empty cell that air from the box's six faces cannot reach is filled: the through-empty flood of the whole box, uncapped in effect.
    void seal() {
        if (!m_opt.seal) return;
        const uint32_t faces = BLOK_FLOOD_SEED_FACE(0) | BLOK_FLOOD_SEED_FACE(1) | BLOK_FLOOD_SEED_FACE(2) | BLOK_FLOOD_SEED_FACE(3) | BLOK_FLOOD_SEED_FACE(4) | BLOK_FLOOD_SEED_FACE(5);
        const blok_flood_info info = m_tracer->floodField(nullptr, nullptr, {}, BLOK_FLOOD_MAX_STEPS, faces);
        const uint64_t filled = m_tracer->editByFlood(BLOK_FLOOD_FILL_UNREACHED, 0, 1.0f, m_opt.seal_material);
        std::cout << "seal: " << filled << " voxels filled, farthest " << info.farthest << "\n";
    }
    // The first model of a .vox file in the local lattice of the models here (VOX z is up -> local y), its palette imported as materials.
    // (imported == false: nothing is imported, a voxel's id is its palette index)
    void loadVoxModel(const std::string& path, std::vector<int32_t>& xyz, std::vector<uint32_t>& ids, uint32_t size[3], bool imported = true) {
        char err[512] = {0};
        blok_vox* vox = nullptr;
        if (blok_vox_load_file(path.c_str(), &vox, err, sizeof(err)) != BLOK_OK) throw std::runtime_error("Failed to load VOX: " + std::string(err));
        uint32_t n = 0, palette[256];
        if (blok_vox_model_count(vox) == 0 || blok_vox_model_info(vox, 0, size, &n) != BLOK_OK || n == 0) { blok_vox_free(vox); throw std::runtime_error("the VOX holds no voxels: " + path); }
        if (imported) blok_vox_import_materials(vox, m_materials.handle(), palette);
        else for (uint32_t k = 0; k < 256u; ++k) palette[k] = k;
        const uint8_t* v = blok_vox_model_voxels(vox, 0);
        xyz.resize(3u * n);
        ids.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            xyz[3 * i] = v[4 * i]; xyz[3 * i + 1] = v[4 * i + 2]; xyz[3 * i + 2] = v[4 * i + 1];
            ids[i] = palette[v[4 * i + 3]];
        }
        blok_vox_free(vox);
    }
    // Each --paste model turned about +y around the centre of its voxels' box, scaled, and resampled into the volume with that centre at the
    // given world point: forward = T(position) Ry(yaw) S(scale) T(-centre), inverted and rounded by blok_affine_from_matrix.
    void paste() {
        for (const Options::Paste& P : m_opt.paste) {
            std::vector<int32_t> xyz;
            std::vector<uint32_t> ids;
            uint32_t size[3] = {0, 0, 0};
            loadVoxModel(P.path, xyz, ids, size);
            int32_t lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
            for (size_t i = 0; i < ids.size(); ++i)
                for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], xyz[3 * i + a]); hi[a] = std::max(hi[a], xyz[3 * i + a] + 1); }
            const double pivot[3] = {(lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0, (lo[2] + hi[2]) / 2.0};
            const double yaw = P.yaw_deg * (3.14159265358979323846 / 180.0), cy = std::cos(yaw), sy = std::sin(yaw), s = P.scale;
            const double r[3][3] = {{cy, 0.0, sy}, {0.0, 1.0, 0.0}, {-sy, 0.0, cy}};
            double forward[12];
            for (int i = 0; i < 3; ++i) {
                const double row[3] = {s * r[i][0], s * r[i][1], s * r[i][2]};
                for (int j = 0; j < 3; ++j) forward[4 * i + j] = row[j];
                forward[4 * i + 3] = P.position[i] - (row[0] * pivot[0] + row[1] * pivot[1] + row[2] * pivot[2]);
            }
            blok_affine record;
            if (blok_affine_from_matrix(forward, &record) != BLOK_OK) throw std::runtime_error("--paste: the map has no record (blok_affine_from_matrix): SCALE must be at least 1/64");
            record.model = m_tracer->createModel(xyz, ids);
            const uint64_t written = m_tracer->stampAffine({record}, nullptr, nullptr, BLOK_STAMP_SET, 1.0f);
            std::cout << "paste: " << P.path << ": " << ids.size() << " voxels turned " << P.yaw_deg << " degrees, scaled " << P.scale << " -> " << written << " voxels written\n";
        }
    }
    // Each --pose model uploaded and given its pose: --paste's forward map (T(position) Ry(yaw) S(scale) T(-centre)) inverted and rounded by
    // blok_pose_from_matrix about the centre of the voxels' box.
    blok_pose poseOf(size_t i, double yaw_deg) const {
        const Options::Paste& P = m_opt.posed[i];
        const double* pivot = m_posePivots[i].data();
        const double yaw = yaw_deg * (3.14159265358979323846 / 180.0), cy = std::cos(yaw), sy = std::sin(yaw), s = P.scale;
        const double r[3][3] = {{cy, 0.0, sy}, {0.0, 1.0, 0.0}, {-sy, 0.0, cy}};
        double forward[12];
        for (int k = 0; k < 3; ++k) {
            const double row[3] = {s * r[k][0], s * r[k][1], s * r[k][2]};
            for (int j = 0; j < 3; ++j) forward[4 * k + j] = row[j];
            forward[4 * k + 3] = P.position[k] - (row[0] * pivot[0] + row[1] * pivot[1] + row[2] * pivot[2]);
        }
        blok_pose pose;
        if (blok_pose_from_matrix(forward, pivot, m_poseModels[i], &pose) != BLOK_OK)
            throw std::runtime_error("--pose: the map has no pose (blok_pose_from_matrix): SCALE must be at least 1/1024 and the position within 2^20");
        return pose;
    }
    // --pose-motion: drawn frame `frame` with every pose turned to its YAW_DEG + frame * --pose-spin, by the entry that tracks them
    const std::vector<uint32_t>& drawPoseMotionFrame(uint32_t frame) {
        for (size_t i = 0; i < m_poses.size(); ++i) m_poses[i] = poseOf(i, m_opt.posed[i].yaw_deg + frame * m_opt.pose_spin);
        const blok_camera c = m_camera.basis(m_opt.width, m_opt.height);
        const float cam[14] = {c.pos[0], c.pos[1], c.pos[2], c.fwd[0], c.fwd[1], c.fwd[2], c.right[0], c.right[1], c.right[2], c.up[0], c.up[1], c.up[2], c.tan_half_fov, c.aspect};
        std::printf("pose: frame %u camera", frame);
        for (float v : cam) std::printf(" %.9g", v);
        std::printf("\n");
        std::fflush(stdout);
        return m_tracer->drawFrameRtPosedMotion(m_camera, m_instances, m_poses, m_opt.spp);
    }
    void loadPoses(bool imported) {
        for (const Options::Paste& P : m_opt.posed) {
            std::vector<int32_t> xyz;
            std::vector<uint32_t> ids;
            uint32_t size[3] = {0, 0, 0};
            loadVoxModel(P.path, xyz, ids, size, imported);
            int32_t lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
            for (size_t i = 0; i < ids.size(); ++i)
                for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], xyz[3 * i + a]); hi[a] = std::max(hi[a], xyz[3 * i + a] + 1); }
            m_posePivots.push_back({(lo[0] + hi[0]) / 2.0, (lo[1] + hi[1]) / 2.0, (lo[2] + hi[2]) / 2.0});
            m_poseModels.push_back(m_tracer->createModel(xyz, ids));
            m_poses.push_back(poseOf(m_poses.size(), P.yaw_deg));
            std::cout << "pose: " << P.path << ": " << ids.size() << " voxels turned " << P.yaw_deg << " degrees, scaled " << P.scale << "\n";
        }
        if (!m_poses.empty()) m_tracer->checkPoses(m_poses);
    }
    const std::vector<uint32_t>& drawPosed() {
        const size_t n = static_cast<size_t>(m_opt.width) * m_opt.height;
        m_populatedHits.resize(n);
        m_populatedFrame.resize(n);
        m_poseIds.resize(n);
        m_tracer->tracePrimaryPosed(m_camera, m_instances, m_poses, m_populatedHits.data(), m_populatedFrame.data(), m_poseIds.data());
        return m_populatedFrame;
    }
    // The listed .vox models scattered over the terrain's grass: the column field of the whole box, then the table — kept for the frames, or baked.
    void populate(const blok_terrain_params& terrain) {
        if (m_opt.populate.empty()) return;
        if (m_opt.populate.size() > BLOK_SCATTER_MAX_ENTRIES) throw std::runtime_error("--populate takes at most 16 models");
        std::vector<blok_scatter_entry> entries;
        for (const std::string& path : m_opt.populate) {
            std::vector<int32_t> xyz;
            std::vector<uint32_t> ids;
            uint32_t size[3] = {0, 0, 0};
            loadVoxModel(path, xyz, ids, size);
            blok_scatter_entry e{};
            e.model = m_tracer->createModel(xyz, ids);
            m_populateModels.push_back(e.model);
            e.weight = 1u;
            e.anchor[0] = static_cast<int32_t>(size[0] / 2u); e.anchor[1] = 0; e.anchor[2] = static_cast<int32_t>(size[1] / 2u);
            entries.push_back(e);
        }
        const blok_columns_info columns = m_tracer->columnField(nullptr, nullptr, 1u, 0u);
        blok_scatter_params sp{};
        sp.seed = m_opt.terrain_seed; sp.flags = BLOK_SCATTER_ROTATE | BLOK_SCATTER_MIRROR;
        sp.cell_log2 = 4u; sp.probability = 40000u; sp.surface_material = terrain.surface_material;
        sp.min_y = INT32_MIN; sp.max_y = INT32_MAX;
        sp.radius = 1u; sp.max_rise = 1u; sp.max_drop = 1u;
        const blok_scatter_info info = m_tracer->scatterModels(sp, entries);
        m_instances = m_tracer->downloadScatter();
        if (blok_hip_check_instances(m_tracer->handle(), m_instances.data(), static_cast<uint32_t>(m_instances.size())) != BLOK_OK)
            throw std::runtime_error(std::string("--populate: ") + blok_hip_last_error(m_tracer->handle()));
        std::cout << "populate: " << entries.size() << " models over " << columns.n_hit << " of " << columns.n_columns << " columns, " << info.n_cells << " cells, "
                  << info.n_placed << " placed, rejected " << info.n_rejected[0] << " " << info.n_rejected[1] << " " << info.n_rejected[2] << " " << info.n_rejected[3] << " "
                  << info.n_rejected[4];
        if (m_opt.bake) {
            std::cout << ", baked " << m_tracer->stampModels(m_instances, BLOK_STAMP_SET, 1.0f) << " voxels";
            m_instances.clear();
        }
        std::cout << "\n";
    }
    // The frame over the world plus the scattered table, as RGBA8.
    const std::vector<uint32_t>& drawPopulated() {
        const blok_camera c = m_camera.basis(m_opt.width, m_opt.height);
        m_populatedHits.resize(static_cast<size_t>(m_opt.width) * m_opt.height);
        m_populatedFrame.resize(m_populatedHits.size());
        if (blok_hip_trace_primary_instanced(m_tracer->handle(), &c, 0, 0, m_opt.width, m_opt.height, m_instances.data(), static_cast<uint32_t>(m_instances.size()),
                                             m_populatedHits.data(), m_populatedFrame.data(), nullptr) != BLOK_OK)
            throw std::runtime_error(std::string("HipTracer: ") + blok_hip_last_error(m_tracer->handle()));
        return m_populatedFrame;
    }
    // Only the shell within the squared distance --hollow of empty space stays: the to-empty field of the whole box, thresholded.
    void hollow() {
        if (m_opt.hollow < 0) return;
        const uint32_t d2 = static_cast<uint32_t>(m_opt.hollow);
        uint32_t radius = 0;
        while (radius * radius < d2) ++radius;
        const blok_distance_info info = m_tracer->distanceField(nullptr, nullptr, radius, true);
        const uint64_t cleared = m_tracer->editByDistance(BLOK_DISTANCE_HOLLOW, d2);
        std::cout << "hollow: " << cleared << " voxels cleared, " << info.n_near + info.n_far - cleared << " left\n";      // (the filled cells are those with D > 0)
    }
    // The rule of --rule or --smooth stepped over the whole box.
    void automaton() {
        if (!m_opt.rule.steps) return;
        const blok_automaton_info info = m_tracer->volumeAutomaton(m_opt.rule);
        std::cout << "rule: " << info.steps_run << " steps run, " << info.n_born << " voxels born, " << info.n_died << " died, " << info.n_filled << " left\n";
    }
    // The far-field copy of the terrain in place of the terrain: level K of the whole box's pyramid, installed as a dense world of voxel size 2^K.
    void lod() {
        if (!m_opt.lod) return;
        if (!m_instances.empty()) throw std::runtime_error("--lod shows the coarse world alone: --populate needs --bake with it");
        const uint32_t K = m_opt.lod;
        const blok_lod_info info = m_tracer->reduceVolume(nullptr, nullptr, K, BLOK_LOD_VOTE_EXPOSED);
        const blok_lod_level& L = info.level[K - 1];
        const std::vector<uint16_t> n = m_tracer->downloadLod<uint16_t>(K, 0);
        std::vector<uint32_t> ids = m_tracer->downloadLod<uint32_t>(K, 2);
        uint64_t voxels = 0;
        for (size_t i = 0; i < ids.size(); ++i) {
            if (n[i] < m_opt.lod_min) ids[i] = 0u;            // the dense form: 0 = empty ...
            else { ++voxels; if (!ids[i]) ids[i] = 1u; }      // ... so a filled cell whose voted id is 0 takes the first material
        }
        std::cout << "lod: level " << K << ": " << L.n_filled << " of " << L.n_cells << " cells filled, " << L.n_exposed << " exposed, " << voxels << " voxels at min "
                  << m_opt.lod_min << "\n";
        if (!voxels) throw std::runtime_error("--lod: no coarse cell holds that many voxels");
        const auto must = [&](int rc) { if (rc != BLOK_OK) throw std::runtime_error(std::string("HipTracer: ") + blok_hip_last_error(m_tracer->handle())); };
        must(blok_hip_volume_destroy(m_tracer->handle()));
        m_tracer->setVoxelSize(static_cast<float>(1u << K));
        const std::vector<blok_material> materials = m_materials.packForGpu();
        must(blok_hip_upload_dense(m_tracer->handle(), ids.data(), L.cext[0], L.cext[1], L.cext[2], L.clo, materials.data(), materials.size()));
        const blok_world_stats s = m_tracer->worldStats();
        std::cout << "world: " << s.n_voxels << " voxels of size " << (1u << K) << ", " << s.n_tree_nodes << " tree nodes, " << s.levels << " levels\n";
    }
    // A brush dragged through the points of --stroke: the capsules from each point to the next, applied as one table in one pass.
    void stroke() {
        if (m_opt.stroke.empty()) return;
        const uint32_t op = m_opt.stroke_op;
        const bool writes_id = op == BLOK_SHAPE_SET || op == BLOK_SHAPE_KEEP || op == BLOK_SHAPE_PAINT;
        const std::vector<blok_shape> table = blok::HipTracer::strokeShapes(m_opt.stroke, m_opt.stroke_radius, op, writes_id ? 1u : 0u, op == BLOK_SHAPE_SUBTRACT ? 0.0f : 1.0f);
        const uint64_t written = m_tracer->applyShapes(table);
        std::cout << "stroke: " << table.size() << " capsules, " << written << " voxels written\n";
    }
    // The whole box as a sparse brick stream: encoded on the device, downloaded, written as a .bvol file.
    void saveVolume() {
        if (m_opt.save_volume.empty()) return;
        m_tracer->encodeBricks();
        const blok::HipTracer::BrickStream s = m_tracer->downloadBricks();
        char err[512] = {0};
        if (blok_bricks_write_file(m_opt.save_volume.c_str(), &s.info, s.records.data(), s.density.data(), s.material.data(), err, sizeof(err)) != BLOK_OK)
            throw std::runtime_error(std::string("Failed to save volume: ") + err);
        const uint64_t bytes = 8u + sizeof(blok_bricks_info) + s.records.size() * sizeof(blok_brick_record) + (s.density.size() + s.material.size()) * sizeof(uint32_t);
        std::cout << "volume saved: " << s.info.n_bricks << " bricks, " << s.info.n_voxels << " voxels, " << bytes << " bytes\n";
    }
    // The mesh's bounding box fitted into obj_size voxels (half a voxel from the faces), voxelized into a volume of that box, rebuilt.
    void initObj() {
        if (m_opt.devices.size() > 1) throw std::runtime_error("--obj renders on one device");
        char err[512] = {0};
        blok_mesh* mesh = nullptr;
        if (blok_obj_load_file(m_opt.obj.c_str(), m_materials.handle(), &mesh, err, sizeof(err)) != BLOK_OK)
            throw std::runtime_error(std::string("Failed to load OBJ: ") + err);
        const size_t nv = blok_mesh_vertex_count(mesh), nt = blok_mesh_triangle_count(mesh);
        std::vector<float> pos(blok_mesh_positions(mesh), blok_mesh_positions(mesh) + 3 * nv);
        std::vector<uint32_t> tri(blok_mesh_triangles(mesh), blok_mesh_triangles(mesh) + 3 * nt);
        std::vector<uint32_t> mat(blok_mesh_materials(mesh), blok_mesh_materials(mesh) + nt);
        blok_mesh_free(mesh);
        if (nt == 0) throw std::runtime_error("the OBJ has no faces");
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (size_t i = 0; i < nv; ++i)
            for (int a = 0; a < 3; ++a) { lo[a] = std::min<double>(lo[a], pos[3 * i + a]); hi[a] = std::max<double>(hi[a], pos[3 * i + a]); }
        const double extent = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
        const double n = m_opt.obj_size, scale = extent > 0 ? (n - 1.0) / extent : 1.0;
        for (size_t i = 0; i < nv; ++i)
            for (int a = 0; a < 3; ++a) pos[3 * i + a] = static_cast<float>((pos[3 * i + a] - (lo[a] + hi[a]) / 2.0) * scale + n / 2.0);
        const int32_t origin[3] = {0, 0, 0};
        m_tracer->createVolume(origin, m_opt.obj_size, m_opt.obj_size, m_opt.obj_size);
        const uint64_t written = m_tracer->voxelizeMesh(pos, tri, mat, 1, 1.0f, m_opt.solid);
        seal();
        hollow();
        automaton();
        stroke();
        m_tracer->rebuildVolume(gpuMaterials());
        const blok_world_stats s = m_tracer->worldStats();
        std::cout << "mesh: " << nv << " vertices, " << nt << " triangles -> " << written << " voxels written (" << (m_opt.solid ? "solid" : "surface")
                  << "); world: " << s.n_voxels << " voxels, " << s.n_tree_nodes << " tree nodes, " << s.levels << " levels\n";
        const float eye[3] = {static_cast<float>(-0.35 * n), static_cast<float>(1.15 * n), static_cast<float>(-0.45 * n)};
        float f[3] = {static_cast<float>(n / 2) - eye[0], static_cast<float>(n / 2) - eye[1], static_cast<float>(n / 2) - eye[2]};
        const float len = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
        for (int a = 0; a < 3; ++a) { f[a] /= len; m_camera.position[a] = eye[a]; }
        m_camera.pitch = std::asin(f[1]) * 57.29577951308232f;
        m_camera.yaw = std::atan2(f[2], f[0]) * 57.29577951308232f;
    }
    // The whole box of the resident volume as merged quads, written as an OBJ beside the library's albedos.
    void exportObj() {
        if (m_opt.export_obj.empty()) return;
        uint64_t faces = 0;
        const std::vector<blok_quad> quads = m_tracer->extractQuads(nullptr, nullptr, false, &faces);
        char err[512] = {0};
        if (blok_quads_write_obj(m_opt.export_obj.c_str(), quads.data(), quads.size(), m_materials.handle(), err, sizeof(err)) != BLOK_OK)
            throw std::runtime_error(std::string("Failed to write OBJ: ") + err);
        std::cout << "surface: " << faces << " exposed faces -> " << quads.size() << " quads (" << quads.size() * sizeof(blok_quad) / 1e6
                  << " MB) -> " << m_opt.export_obj << "\n";
    }
    // The connected components of the whole box: their number, the largest, and those that do not reach the box's floor.
    void components() {
        if (!m_opt.components) return;
        uint64_t voxels = 0, largest = 0, floating = 0, floating_voxels = 0;
        const std::vector<blok_component> records = m_tracer->labelComponents(nullptr, nullptr, &voxels);
        for (const blok_component& c : records) {
            largest = std::max<uint64_t>(largest, c.n_voxels);
            if (!(c.touches & (1u << 3))) { ++floating; floating_voxels += c.n_voxels; }
        }
        std::cout << "components: " << records.size() << " over " << voxels << " voxels, largest " << largest << " voxels, " << floating
                  << " not touching the floor (" << floating_voxels << " voxels)\n";
    }
    // Floating pieces fall: label, lift each piece that does not reach the floor out of the volume (lowest first), sweep it down against
    // what remains, stamp it where it comes to rest; again until nothing floats (a piece may land on one that falls later in the pass).
    void settle() {
        if (!m_opt.settle) return;
        const uint32_t height = m_opt.terrain ? m_opt.terrain_size : m_opt.obj_size;
        uint64_t pieces = 0, voxels = 0, total = 0, longest = 0;
        for (int pass = 0; pass < 8; ++pass) {
            std::vector<blok_component> floating;
            for (const blok_component& c : m_tracer->labelComponents())
                if (!(c.touches & (1u << 3))) floating.push_back(c);
            if (floating.empty()) break;
            std::sort(floating.begin(), floating.end(), [](const blok_component& a, const blok_component& b) {
                return a.lo[1] != b.lo[1] ? a.lo[1] < b.lo[1] : a.label < b.label; });
            for (const blok_component& c : floating) {
                blok_instance piece{};
                uint64_t n = 0;
                piece.model = m_tracer->captureComponent(c.label, true, piece.offset, &n);
                piece.axis[0] = 0; piece.axis[1] = 1; piece.axis[2] = 2;
                const blok_sweep_result fall = m_tracer->sweepModels({piece}, 3u, height, true)[0];
                piece.offset[1] -= static_cast<int32_t>(fall.travel);
                m_tracer->stampModels({piece}, BLOK_STAMP_SET, 1.0f);
                m_tracer->destroyModel(piece.model);
                ++pieces; voxels += n; total += fall.travel; longest = std::max<uint64_t>(longest, fall.travel);
            }
        }
        m_tracer->rebuildVolume(gpuMaterials());
        uint64_t left = 0;
        const std::vector<blok_component> records = m_tracer->labelComponents();
        for (const blok_component& c : records) left += !(c.touches & (1u << 3));
        std::cout << "settle: " << pieces << " pieces, " << voxels << " voxels, travel " << total << " in total, longest " << longest << "; "
                  << records.size() << " components after, " << left << " not touching the floor\n";
    }
    // The library's materials as the rebuilds install them: --glow ID[:R,G,B] gives material ID that emission (four times its albedo without one).
    std::vector<blok_material> gpuMaterials() {
        std::vector<blok_material> table = m_materials.packForGpu();
        for (const Options::Glow& g : m_opt.glow) {
            if (g.id >= table.size()) throw std::runtime_error("--glow " + std::to_string(g.id) + ": the material table has " + std::to_string(table.size()) + " entries");
            for (int a = 0; a < 3; ++a) table[g.id].emission[a] = g.has_rgb ? g.rgb[a] : 4.0f * table[g.id].albedo[a];
        }
        return table;
    }
    // --lights: the installed world's emissive faces become the light table every path-traced frame samples (behind the last rebuild: a
    // rebuild clears the table): the whole box as quads, then the table from them on the device.
    void installLights() {
        if (!m_opt.lights) return;
        if (!(m_opt.terrain || !m_opt.obj.empty() || !m_opt.load_volume.empty())) throw std::runtime_error("--lights needs a resident volume: --terrain, --obj or --load-volume");
        uint64_t quads = 0, faces = 0;
        if (blok_hip_volume_extract_quads(m_tracer->handle(), nullptr, nullptr, 0u, &quads, &faces) != BLOK_OK)
            throw std::runtime_error(std::string("--lights: ") + blok_hip_last_error(m_tracer->handle()));
        const blok_lights_info info = m_tracer->lightsFromQuads();
        std::cout << "lights: " << info.n << " rectangles, " << info.n_faces << " faces, " << info.n_owned << " materials (of " << quads << " quads, " << faces << " exposed faces)\n";
        if (!m_opt.has_light_grid) return;
        if (info.n == 0) throw std::runtime_error("--light-grid: the light table is empty (no emissive face in the volume: --glow ID)");
        const blok_light_grid_info grid = m_tracer->buildLightGrid(m_opt.light_grid[0], m_opt.light_grid[1], m_opt.light_grid[2]);
        std::cout << "light grid: " << grid.n_cells << " cells (" << grid.dim[0] << " x " << grid.dim[1] << " x " << grid.dim[2] << " of " << (1u << grid.cell_log2) << " voxels, reach "
                  << grid.reach << ", share " << grid.share << "/256), " << grid.n_nonempty << " with a list, " << grid.n_items << " items, the longest list " << grid.max_items << "\n";
    }
    // --model-lights: every loaded model's own light table (behind the last rebuild: a new material table drops them), and what the scattered
    // table makes of them.
    void installModelLights() {
        if (!m_opt.model_lights) return;
        if (m_instances.empty()) throw std::runtime_error("--model-lights: nothing is placed (--populate scattered no model over this terrain)");
        uint64_t faces = 0;
        for (const uint32_t model : m_populateModels) faces += m_tracer->modelLights(model).n;
        const blok_instance_lights_info info = m_tracer->instanceLightsInfo(m_instances);
        std::cout << "model lights: " << m_populateModels.size() << " models, " << faces << " faces; " << m_instances.size() << " instances, " << info.n_lit << " lit, "
                  << info.a_inst << " faces in the world" << (info.disabled ? " (disabled: 2^32 faces or more)" : "") << "\n";
    }
    void update() {
        using clock = std::chrono::steady_clock;
        installLights();
        installModelLights();
        for (uint32_t f = 0; f < m_opt.frames; ++f) {
            const auto t0 = clock::now();
            m_tracer->beginFrame();
            if (m_multi) m_multi->drawFrame(m_camera, m_multiFrame);
            else if (m_opt.pose_motion) drawPoseMotionFrame(f);
            else if (m_opt.rt_posed) m_tracer->drawFrameRtPosed(m_camera, m_instances, m_poses, m_opt.spp);
            else if (m_opt.rt && (m_opt.far || m_opt.model_lights)) m_tracer->drawFrameRTInstanced(m_camera, m_instances, m_opt.spp);
            else if (m_opt.rt) m_tracer->drawFrameRT(m_camera, m_opt.spp);
            else if (!m_poses.empty()) m_tracer->drawFramePosed(m_camera, m_instances, m_poses);
            else if (!m_instances.empty()) m_tracer->drawFrameInstanced(m_camera, m_instances);
            else m_tracer->drawFrame(m_camera);
            m_tracer->endFrame();
            const double ms = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
            if (m_multi) std::cout << "frame " << f << ": " << ms << " ms (" << m_multi->deviceCount() << " ranks, incl. device->host copy of the RGBA8 frame)\n";
            else if (m_opt.rt || m_opt.rt_posed) std::cout << "frame " << f << ": " << ms << " ms (path trace " << m_opt.spp << " spp, denoise, TAA, tonemap, sharpen; incl. device->host copy)\n";
            else std::cout << "frame " << f << ": " << ms << " ms (incl. device->host copy of "
                           << m_tracer->hits().size() * sizeof(blok_hit) / 1e6 << " MB)\n";
            if (f + 1 < m_opt.frames || !(m_opt.rt || m_opt.rt_posed)) m_camera.processKeyboard('W', 0.016f);
        }
        const auto& single = m_opt.pose_motion ? drawPoseMotionFrame(m_opt.frames)
                             : m_opt.rt_posed ? m_tracer->drawFrameRtPosed(m_camera, m_instances, m_poses, m_opt.spp)
                             : m_opt.rt && (m_opt.far || m_opt.model_lights) ? m_tracer->drawFrameRTInstanced(m_camera, m_instances, m_opt.spp)
                             : m_opt.rt ? m_tracer->drawFrameRT(m_camera, m_opt.spp) : !m_poses.empty() ? drawPosed() : !m_instances.empty() ? drawPopulated() : m_tracer->drawFrameRgba8(m_camera);
        if (m_multi) {                                       // the partitioned frame must be the single-device frame
            m_multi->drawFrame(m_camera, m_multiFrame);
            size_t differ = 0;
            for (size_t i = 0; i < single.size(); ++i) differ += single[i] != m_multiFrame[i];
            std::cout << "multi-device frame vs single-device frame: " << differ << " pixels differ\n";
            if (differ) throw std::runtime_error("multi-device frame differs from the single-device frame");
        }
        farReport();
        if (m_opt.has_light_grid) {                         // the camera of the written frame, exactly (%.9g round-trips a float)
            const blok_camera c = m_camera.basis(m_opt.width, m_opt.height);
            const float cam[14] = {c.pos[0], c.pos[1], c.pos[2], c.fwd[0], c.fwd[1], c.fwd[2], c.right[0], c.right[1], c.right[2], c.up[0], c.up[1], c.up[2], c.tan_half_fov, c.aspect};
            std::printf("light grid: camera");
            for (float v : cam) std::printf(" %.9g", v);
            std::printf("\n");
            std::fflush(stdout);
        }
        if (m_opt.model_lights) {                           // the camera of the written frame, exactly (%.9g round-trips a float)
            const blok_camera c = m_camera.basis(m_opt.width, m_opt.height);
            const float cam[14] = {c.pos[0], c.pos[1], c.pos[2], c.fwd[0], c.fwd[1], c.fwd[2], c.right[0], c.right[1], c.right[2], c.up[0], c.up[1], c.up[2], c.tan_half_fov, c.aspect};
            std::printf("model lights: camera");
            for (float v : cam) std::printf(" %.9g", v);
            std::printf("\n");
            std::fflush(stdout);
        }
        if (!m_poses.empty()) {                             // the camera of the written frame, exactly (%.9g round-trips a float), and who won it
            const blok_camera c = m_camera.basis(m_opt.width, m_opt.height);
            const float cam[14] = {c.pos[0], c.pos[1], c.pos[2], c.fwd[0], c.fwd[1], c.fwd[2], c.right[0], c.right[1], c.right[2], c.up[0], c.up[1], c.up[2], c.tan_half_fov, c.aspect};
            std::printf("pose: camera");
            for (float v : cam) std::printf(" %.9g", v);
            std::printf("\n");
            std::fflush(stdout);
            if (!m_opt.rt_posed) {                           // (the path-traced chain keeps no id plane)
                size_t won = 0;
                for (uint32_t id : m_poseIds) won += id != BLOK_INSTANCE_NONE && (id & BLOK_POSE_ID) != 0u;
                std::cout << "pose: poses won " << won << " of " << m_poseIds.size() << " pixels\n";
            }
        }
        const auto& px = m_multi ? m_multiFrame : single;
        std::ofstream ppm(m_opt.out, std::ios::binary);
        ppm << "P6\n" << m_opt.width << " " << m_opt.height << "\n255\n";
        for (uint32_t p : px) { const char rgb[3] = {char(p & 255), char((p >> 8) & 255), char((p >> 16) & 255)}; ppm.write(rgb, 3); }
        std::cout << "wrote " << m_opt.out << "\n";
    }
    void shutdown() { if (m_tracer) m_tracer->shutdown(); }

    blok::GraphicsApi m_backend;
    Options m_opt;
    blok::ChunkManager m_mgr;
    blok::MaterialLibrary m_materials;
    blok::WorldSvoGpu m_world;                     // App owns the world, the tracer its device copy (app.hpp:40)
    blok::Camera m_camera;
    std::unique_ptr<blok::HipTracer> m_tracer;
    std::unique_ptr<blok::HipMultiTracer> m_multi;
    std::vector<uint32_t> m_multiFrame;
    std::vector<uint32_t> m_populateModels;        // --populate: the ids of the models it loaded, in the order of the list
    std::vector<blok_instance> m_instances;        // --populate: the scattered table (empty once baked); --far: the ring of coarse copies
    std::vector<blok_hit> m_populatedHits;
    std::vector<uint32_t> m_populatedFrame;
    std::vector<blok_pose> m_poses;                // --pose FILE.vox@...: the posed models, in the order given
    std::vector<uint32_t> m_poseIds;
    std::vector<std::array<double, 3>> m_posePivots;   // ... each one's pivot (the centre of its voxels' box) and model, for --pose-motion's turns
    std::vector<uint32_t> m_poseModels;
};

}  // namespace

// --stroke's argument: points separated by ':', the last followed by the radius and, if given, the operation.  Numbers are multiples of
// one half and become half-voxel units.
static bool parseStroke(const std::string& arg, Options& opt) {
    const auto half = [](const std::string& s, int32_t* out) {
        char* end = nullptr;
        const double v = 2.0 * std::strtod(s.c_str(), &end);
        if (end == s.c_str() || *end || !(std::fabs(v) < 1.0e6) || v != std::floor(v)) return false;
        *out = static_cast<int32_t>(v);
        return true;
    };
    std::vector<std::string> points;
    for (std::string rest = arg; ;) {
        const size_t c = rest.find(':');
        points.push_back(rest.substr(0, c));
        if (c == std::string::npos) break;
        rest = rest.substr(c + 1);
    }
    for (size_t k = 0; k < points.size(); ++k) {
        std::vector<std::string> f;
        for (std::string rest = points[k]; ;) {
            const size_t c = rest.find(',');
            f.push_back(rest.substr(0, c));
            if (c == std::string::npos) break;
            rest = rest.substr(c + 1);
        }
        const bool last = k + 1 == points.size();
        if (last ? (f.size() != 4 && f.size() != 5) : f.size() != 3) return false;
        std::array<int32_t, 3> p{};
        for (int a = 0; a < 3; ++a) if (!half(f[a], &p[a])) return false;
        opt.stroke.push_back(p);
        if (!last) continue;
        int32_t r = 0;
        if (!half(f[3], &r) || r < 0) return false;
        opt.stroke_radius = static_cast<uint32_t>(r);
        if (f.size() == 5) {
            static const char* const kNames[] = {"set", "keep", "erase", "paint", "", "add", "subtract"};      // = BLOK_SHAPE_SET .. _SUBTRACT; REPLACE takes a match
            uint32_t op = 0;
            while (op < 7u && (f[4] != kNames[op] || !kNames[op][0])) ++op;
            if (op == 7u) return false;
            opt.stroke_op = op;
        }
    }
    return true;
}

int main(int argc, char** argv) {
    Options opt;
    for (int i = 1; i < argc; ++i) {
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", argv[i]); std::exit(2); } return argv[++i]; };
        if (!std::strcmp(argv[i], "--n")) opt.n = std::strtoul(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--size")) { if (std::sscanf(next(), "%ux%u", &opt.width, &opt.height) != 2) return 2; }
        else if (!std::strcmp(argv[i], "--pose")) {
            const std::string arg = next();
            const size_t at = arg.rfind('@');
            if (at == std::string::npos) { opt.pose = std::atoi(arg.c_str()); continue; }      // a bare number: the camera pose
            Options::Paste P{};
            P.scale = 1.0;
            char tail = 0;
            const char* spec = arg.c_str() + at + 1;
            bool whole = at != 0 && std::sscanf(spec, "%lf,%lf,%lf,%lf%c", &P.position[0], &P.position[1], &P.position[2], &P.yaw_deg, &tail) == 4;
            if (!whole) whole = at != 0 && std::sscanf(spec, "%lf,%lf,%lf,%lf,%lf%c", &P.position[0], &P.position[1], &P.position[2], &P.yaw_deg, &P.scale, &tail) == 5;
            if (!whole || !std::isfinite(P.position[0]) || !std::isfinite(P.position[1]) || !std::isfinite(P.position[2]) || !std::isfinite(P.yaw_deg) ||
                !std::isfinite(P.scale) || !(P.scale > 0.0)) {
                std::fprintf(stderr, "--pose takes FILE.vox@X,Y,Z,YAW_DEG[,SCALE] with SCALE > 0 (or a bare number: the camera pose)\n");
                return 2;
            }
            P.path = arg.substr(0, at);
            opt.posed.push_back(P);
        }
        else if (!std::strcmp(argv[i], "--frames")) opt.frames = std::strtoul(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--out")) opt.out = next();
        else if (!std::strcmp(argv[i], "--vox")) opt.vox = next();
        else if (!std::strcmp(argv[i], "--obj")) opt.obj = next();
        else if (!std::strcmp(argv[i], "--obj-size")) opt.obj_size = std::strtoul(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--solid")) opt.solid = true;
        else if (!std::strcmp(argv[i], "--terrain")) { opt.terrain = true; opt.terrain_seed = static_cast<uint32_t>(std::strtoul(next(), nullptr, 0)); }
        else if (!std::strcmp(argv[i], "--terrain-size")) opt.terrain_size = std::strtoul(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--export-obj")) opt.export_obj = next();
        else if (!std::strcmp(argv[i], "--components")) opt.components = true;
        else if (!std::strcmp(argv[i], "--settle")) opt.settle = true;
        else if (!std::strcmp(argv[i], "--seal")) opt.seal = true;
        else if (!std::strcmp(argv[i], "--seal-material")) opt.seal_material = static_cast<uint32_t>(std::atoll(next()));
        else if (!std::strcmp(argv[i], "--hollow")) { opt.hollow = std::atoll(next()); if (opt.hollow < 0 || opt.hollow > 65025) { std::fprintf(stderr, "--hollow takes a squared distance in 0..65025\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--rule") || !std::strcmp(argv[i], "--smooth")) {
            const bool smooth = argv[i][2] == 's';
            const std::string arg = next();
            unsigned nb = 26, survive = 0x7FFE000u, birth = 0x7FFC000u, steps = 0;
            char tail[8] = "";
            const int n = smooth ? std::sscanf(arg.c_str(), "%u%1s", &steps, tail) : std::sscanf(arg.c_str(), "%u,%x,%x,%u,%7s", &nb, &survive, &birth, &steps, tail);
            const bool solid = !smooth && n == 5 && !std::strcmp(tail, "solid");
            opt.rule = blok_automaton_rule{nb, survive, birth, solid ? BLOK_AUTOMATON_BOX_IS_SOLID : 0u, 1.0f, 0u, steps, 0u};
            if ((smooth ? n != 1 : (n != 4 && !solid)) || blok_automaton_check(&opt.rule, nullptr, 0) != BLOK_OK) {
                std::fprintf(stderr, "--rule takes NB,SURVIVE_HEX,BIRTH_HEX,STEPS[,solid] with NB 6, 18 or 26 and 1..255 steps; --smooth takes 1..255 steps\n");
                return 2;
            }
        }
        else if (!std::strcmp(argv[i], "--populate")) { for (std::string list = next(); !list.empty();) { const size_t c = list.find(','); opt.populate.push_back(list.substr(0, c)); list = c == std::string::npos ? "" : list.substr(c + 1); } }
        else if (!std::strcmp(argv[i], "--bake")) opt.bake = true;
        else if (!std::strcmp(argv[i], "--paste")) {
            const std::string arg = next();
            const size_t at = arg.rfind('@');
            Options::Paste P{};
            char tail = 0;
            if (at == std::string::npos || at == 0 ||
                std::sscanf(arg.c_str() + at + 1, "%lf,%lf,%lf,%lf,%lf%c", &P.position[0], &P.position[1], &P.position[2], &P.yaw_deg, &P.scale, &tail) != 5 ||
                !std::isfinite(P.position[0]) || !std::isfinite(P.position[1]) || !std::isfinite(P.position[2]) || !std::isfinite(P.yaw_deg) || !std::isfinite(P.scale) || !(P.scale > 0.0)) {
                std::fprintf(stderr, "--paste takes FILE.vox@X,Y,Z,YAW_DEG,SCALE with SCALE > 0\n");
                return 2;
            }
            P.path = arg.substr(0, at);
            opt.paste.push_back(P);
        }
        else if (!std::strcmp(argv[i], "--lod")) {
            const int got = std::sscanf(next(), "%u,%u", &opt.lod, &opt.lod_min);
            if (got < 1 || opt.lod < 1 || opt.lod > BLOK_LOD_MAX_LEVELS || opt.lod_min < 1 || opt.lod_min > (1u << (3u * opt.lod))) { std::fprintf(stderr, "--lod takes K[,MIN] with K in 1..5 and MIN in 1..8^K\n"); return 2; }
        }
        else if (!std::strcmp(argv[i], "--far")) {
            const int got = std::sscanf(next(), "%u,%u", &opt.far, &opt.far_min);
            if (got < 1 || opt.far < 1 || opt.far > BLOK_LOD_MAX_LEVELS || opt.far_min < 1 || opt.far_min > (1u << (3u * opt.far))) { std::fprintf(stderr, "--far takes K[,MIN] with K in 1..5 and MIN in 1..8^K\n"); return 2; }
        }
        else if (!std::strcmp(argv[i], "--far-direct")) opt.far_direct = true;
        else if (!std::strcmp(argv[i], "--far-rings")) {
            if (std::sscanf(next(), "%u", &opt.far_rings) != 1 || opt.far_rings < 1 || opt.far_rings > 3) { std::fprintf(stderr, "--far-rings takes R in 1..3\n"); return 2; }
            opt.far_direct = true;
        }
        else if (!std::strcmp(argv[i], "--scroll")) { opt.scroll = true; if (std::sscanf(next(), "%d,%d,%d", &opt.scroll_delta[0], &opt.scroll_delta[1], &opt.scroll_delta[2]) != 3) { std::fprintf(stderr, "--scroll takes DX,DY,DZ\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--stroke")) { if (!parseStroke(next(), opt)) { std::fprintf(stderr, "--stroke takes X,Y,Z:X,Y,Z:...,R[,add|subtract|erase|set|keep|paint], coordinates and R in multiples of one half\n"); return 2; } }
        else if (!std::strcmp(argv[i], "--save-volume")) opt.save_volume = next();
        else if (!std::strcmp(argv[i], "--load-volume")) opt.load_volume = next();
        else if (!std::strcmp(argv[i], "--rt")) opt.rt = true;
        else if (!std::strcmp(argv[i], "--rt-posed")) opt.rt_posed = true;
        else if (!std::strcmp(argv[i], "--lights")) opt.lights = true;
        else if (!std::strcmp(argv[i], "--model-lights")) opt.model_lights = true;
        else if (!std::strcmp(argv[i], "--light-grid")) {
            const int got = std::sscanf(next(), "%u,%u,%u", &opt.light_grid[0], &opt.light_grid[1], &opt.light_grid[2]);
            if (got < 1 || opt.light_grid[0] < 2 || opt.light_grid[0] > 12 || opt.light_grid[1] > 3 || opt.light_grid[2] < 1 || opt.light_grid[2] > 255) {
                std::fprintf(stderr, "--light-grid takes C[,R[,SHARE]]: C in 2..12, R in 0..3, SHARE in 1..255\n");
                return 2;
            }
            opt.has_light_grid = true;
        }
        else if (!std::strcmp(argv[i], "--glow")) {
            Options::Glow g{};
            const int got = std::sscanf(next(), "%u:%f,%f,%f", &g.id, &g.rgb[0], &g.rgb[1], &g.rgb[2]);
            if (got != 1 && got != 4) { std::fprintf(stderr, "--glow takes ID or ID:R,G,B\n"); return 2; }
            g.has_rgb = got == 4;
            opt.glow.push_back(g);
        }
        else if (!std::strcmp(argv[i], "--pose-motion")) opt.pose_motion = true;
        else if (!std::strcmp(argv[i], "--pose-spin")) opt.pose_spin = std::atof(next());
        else if (!std::strcmp(argv[i], "--spp")) opt.spp = std::strtoul(next(), nullptr, 10);
        else if (!std::strcmp(argv[i], "--no-rccl")) opt.rccl = false;
        else if (!std::strcmp(argv[i], "--dense-exchange")) opt.dense_exchange = true;
        else if (!std::strcmp(argv[i], "--devices")) { for (const char* p = next(); *p;) { opt.devices.push_back(std::atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; } }
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (!opt.posed.empty() && opt.rt) {
        std::fprintf(stderr, "--pose FILE.vox@... is refused with --rt: posed models are traced in first-hit frames only, the path-traced frame takes no pose table\n");
        return 2;
    }
    if (opt.rt_posed && opt.posed.empty()) {
        std::fprintf(stderr, "--rt-posed path-traces posed models: give at least one --pose FILE.vox@X,Y,Z,YAW_DEG[,SCALE]\n");
        return 2;
    }
    if (opt.rt_posed && (opt.far || !opt.vox.empty() || !opt.obj.empty() || !opt.load_volume.empty() || opt.devices.size() > 1)) {
        std::fprintf(stderr, "--rt-posed path-traces its --pose models over the generated scene or a --terrain, on one device: leave --far, --vox, --obj, --load-volume and --devices out\n");
        return 2;
    }
    if ((opt.pose_motion || opt.pose_spin != 0.0) && !opt.rt_posed) {
        std::fprintf(stderr, "--pose-motion (and --pose-spin) draw --rt-posed's frames with object motion for the poses: give --rt-posed\n");
        return 2;
    }
    if (opt.pose_spin != 0.0 && !opt.pose_motion) {
        std::fprintf(stderr, "--pose-spin turns the poses of --pose-motion's frames: give --pose-motion\n");
        return 2;
    }
    if (opt.lights && !(opt.rt || opt.rt_posed)) { std::fprintf(stderr, "--lights is sampled by the path-traced frames: give --rt or --rt-posed\n"); return 2; }
    if (opt.has_light_grid && !opt.lights) { std::fprintf(stderr, "--light-grid is built over the light table: give --lights\n"); return 2; }
    if (opt.model_lights && (!opt.rt || opt.populate.empty() || opt.bake || opt.far)) {
        std::fprintf(stderr, "--model-lights samples the placed models' emissive faces in the path-traced frames: give --rt and --populate FILE.vox[,...] (without --bake: a baked model is the world's, --lights; without --far)\n");
        return 2;
    }
    if (opt.far_direct && !opt.far) { std::fprintf(stderr, "--far-direct and --far-rings need --far K[,MIN]\n"); return 2; }
    try {
        App app(blok::GraphicsApi::HIP, opt);
        app.run();
    } catch (const std::exception& e) {
        std::cerr << "[FATAL] " << e.what() << std::endl;                                  // main.cpp:19-22
        return 1;
    }
    return 0;
}
