--  art_hip.ads -- thin Ada binding of libart_hip.so (include/art_hip.h), the MI355X render backend.
--  NOTE: written against the reference sources without an Ada toolchain in the build image (no GNAT):
--  syntax-reviewed only.  The same calling sequence is exercised by host/test_main.cpp (C++ mirror).
--
--  Record layouts are Convention C and match include/art_hip.h field for field.
with Interfaces;   use Interfaces;
with Interfaces.C; use Interfaces.C;
with System;
with Interfaces.C.Strings;

package Art_Hip is

  type Float3_C is array (0 .. 2) of aliased C_float;   pragma Convention (C, Float3_C);
  type Float8_C is array (0 .. 7) of aliased C_float;   pragma Convention (C, Float8_C);
  type Float16_C is array (0 .. 15) of aliased C_float; pragma Convention (C, Float16_C);
  type Int6_C is array (0 .. 5) of aliased int;         pragma Convention (C, Int6_C);
  type Normals6_C is array (0 .. 5) of Float3_C;        pragma Convention (C, Normals6_C);

  ART_MAT_NULL    : constant := 0;  ART_MAT_LIGHT  : constant := 1;  ART_MAT_LAMBERT : constant := 2;
  ART_MAT_MIRROR  : constant := 3;  ART_MAT_GLASS  : constant := 4;  ART_MAT_PHONG   : constant := 5;
  ART_LIGHT_RECT  : constant := 0;  ART_LIGHT_SPHERE : constant := 1;
  ART_MESH_REFERENCE_BF : constant := 0;  ART_MESH_CLOSEST : constant := 1;
  ART_LAYOUT_ADA_XY : constant := 0;      ART_LAYOUT_ROW_MAJOR : constant := 1;

  type Art_Material is record          --  materials.ads:58-130 flattened
    kind  : int;
    light : int;
    p     : Float8_C;
  end record;
  pragma Convention (C, Art_Material);

  type Art_Light is record             --  lights.ads:36-55
    shape       : int;
    mat         : int;
    boxMin, boxMax, normal : Float3_C;
    center      : Float3_C;
    radius      : C_float;
    intensity   : Float3_C;
    surfaceArea : C_float;
  end record;
  pragma Convention (C, Art_Light);

  type Art_Sphere is record            --  geometry.ads:21-25
    pos : Float3_C;
    r   : C_float;
    mat : int;
  end record;
  pragma Convention (C, Art_Sphere);

  type Art_Mesh is record              --  geometry.ads:94-101
    mode   : int;
    nverts : int;
    ntris  : int;
    pos, nrm, uv : System.Address;     --  Float3_Array / Float2_Array storage ('Address of element 0)
    idx, matid   : System.Address;     --  Triangle_Array (3 ints each) / MaterialsId_Array
    bbmin, bbmax : Float3_C;
  end record;
  pragma Convention (C, Art_Mesh);

  type Float12_C is array (0 .. 11) of aliased C_float;
  pragma Convention (C, Float12_C);
  type Art_Instance is record          --  embree_connect.cpp:147-184: one instance of a mesh, object -> world 3x4 row-major
    mesh : int;
    m    : Float12_C;
  end record;
  pragma Convention (C, Art_Instance);

  type Art_Scene_Desc is record
    n_spheres   : int;  spheres   : System.Address;
    has_cornell : int;
    cb_min, cb_max : Float3_C;
    cb_mat      : Int6_C;
    cb_nrm      : Normals6_C;
    n_lights    : int;  lights    : System.Address;
    n_materials : int;  materials : System.Address;
    n_meshes    : int;  meshes    : System.Address;
    cam_pos     : Float3_C;
    cam_matrix  : Float16_C;
    n_instances : int;  instances : System.Address;   --  > 0: meshes are object-space prototypes, the geometry is the instance list
  end record;
  pragma Convention (C, Art_Scene_Desc);

  type Art_Pass_Params is record       --  the package variables Render_Pass reads, ray_tracer.ads:20-32
    render_type : int;                 --  Render_Type'Pos (g_rend_type)
    aa_on       : int;
    max_depth   : int;
    vthreads    : int;                 --  Threads_Num
    background  : Float3_C;
    seed        : Unsigned_64;
    layout      : int;
  end record;
  pragma Convention (C, Art_Pass_Params);

  type Art_Hit is record               --  geometry.ads:57-67 flattened (include/art_hip.h ArtHit, 44 bytes)
    t          : C_float;
    is_hit     : int;
    prim_type  : int;                  --  Primitive'Pos: 0 plane, 1 sphere, 2 triangle, 3 quad; -1 miss
    prim_index : int;
    mat_id     : int;
    mat        : int;
    normal     : Float3_C;
    u, v       : C_float;              --  triangle barycentrics (weight of C, weight of B; geometry.adb:245-246)
  end record;
  pragma Convention (C, Art_Hit);

  ART_TRACE_COOP : constant := 0;  ART_TRACE_SIMPLE : constant := 1;
  --  option "bvh_builder": 3 binned SAH on the GPU (default), 0 binned SAH on the host, 1 LBVH, 2 PLOC on the GPU
  ART_BVH_GPU_SAH : constant := 3;  ART_BVH_HOST_SAH : constant := 0;  ART_BVH_GPU_LBVH : constant := 1;  ART_BVH_GPU_PLOC : constant := 2;

  function art_init (device_ordinal : int) return int;
  pragma Import (C, art_init, "art_init");

  --  one process, n GPUs of the node (instead of art_init): ordinals = Null_Address means devices 0 .. n-1
  function art_init_devices (n : int; ordinals : System.Address) return int;
  pragma Import (C, art_init_devices, "art_init_devices");

  function art_upload_scene (scene : access constant Art_Scene_Desc) return int;
  pragma Import (C, art_upload_scene, "art_upload_scene");

  function art_resize (width, height : int) return int;
  pragma Import (C, art_resize, "art_resize");

  function art_render_pass (p : access constant Art_Pass_Params; accum_host : System.Address;
                            screen_host : System.Address; spp_inout : access int) return int;
  pragma Import (C, art_render_pass, "art_render_pass");

  function art_debug_hit_pass (p : access constant Art_Pass_Params; accum_host, screen_host : System.Address;
                               prim_index, mat_id, prim_type : System.Address) return int;
  pragma Import (C, art_debug_hit_pass, "art_debug_hit_pass");

  --  Tuning / build options by name (include/art_hip.h lists them), e.g.
  --    rc := art_set_option (Interfaces.C.Strings.New_String ("bvh_builder"), ART_BVH_HOST_SAH);
  --  BVH options take effect at the next art_upload_scene.
  function art_set_option (name : Interfaces.C.Strings.chars_ptr; value : Interfaces.Integer_64) return int;
  pragma Import (C, art_set_option, "art_set_option");

  --  Scene.Find_Closest_Hit for a list of rays -- SURVEY 8(b)'s "per-ray fallback for debugging": origins / dirs are 3 * n C floats
  --  ('Address of element 0), tfar may be Null_Address (unbounded), hits points at n Art_Hit records, stats may be Null_Address.
  function art_trace_rays (origins, dirs, tfar : System.Address; n : Interfaces.Integer_64; hits : System.Address;
                           kernel : int; stats : System.Address) return int;
  pragma Import (C, art_trace_rays, "art_trace_rays");

  --  First-hit feature buffers of the whole frame (include/art_hip.h ArtAovBuffers, 56 bytes): every component is DEVICE memory of the
  --  library's GPU, row-major, or Null_Address = not wanted.  Of p only aa_on and background are read; hip_stream = Null_Address is the
  --  library's stream.  Stream-ordered like the device ray queries; accum buffer, spp and the statistics are not touched.
  type Art_Aov_Buffers is record
    albedo3f, normal3f : System.Address;            --  3 C floats per pixel
    depth, alpha       : System.Address;            --  1 C float per pixel
    prim_type, prim_index, mat : System.Address;    --  1 int per pixel: Art_Hit's fields for the pixel's ray 0
  end record;
  pragma Convention (C, Art_Aov_Buffers);

  function art_render_aovs_device (p : access constant Art_Pass_Params; buffers : access constant Art_Aov_Buffers;
                                   hip_stream : System.Address) return int;
  pragma Import (C, art_render_aovs_device, "art_render_aovs_device");

  --  The same buffers along the caller's rays (include/art_hip.h states the contract; ArtAovRaysParams 16 bytes, ArtAovRayBuffers 64):
  --  rays are group-major, element g of a plane owns rays g * group .. g * group + group - 1.  origins3f, dirs3f, tnear, tfar and every
  --  component of the buffers are DEVICE memory; tnear, tfar and unwanted planes may be Null_Address.  Needs no viewport.
  type Art_Aov_Rays_Params is record
    group      : int;                               --  1 .. 16
    background : Float3_C;
  end record;
  pragma Convention (C, Art_Aov_Rays_Params);
  type Art_Aov_Ray_Buffers is record
    albedo3f, normal3f, position3f : System.Address;   --  3 C floats per group
    depth, alpha                   : System.Address;   --  1 C float per group
    prim_type, prim_index, mat     : System.Address;   --  1 int per group: Art_Hit's fields for the group's ray 0
  end record;
  pragma Convention (C, Art_Aov_Ray_Buffers);
  function art_aovs_rays_device (p : access constant Art_Aov_Rays_Params; origins3f, dirs3f, tnear, tfar : System.Address;
                                 n_rays : Interfaces.Integer_64; buffers : access constant Art_Aov_Ray_Buffers;
                                 hip_stream : System.Address) return int;
  pragma Import (C, art_aovs_rays_device, "art_aovs_rays_device");
  --  The frame's camera rays into DEVICE memory: ray s of pixel q at q * K + s, K = 4 with p.aa_on, else 1; 3 C floats per ray in each array.
  function art_camera_rays_device (p : access constant Art_Pass_Params; origins3f, dirs3f : System.Address;
                                   hip_stream : System.Address) return int;
  pragma Import (C, art_camera_rays_device, "art_camera_rays_device");

  --  The same call with a motion plane (3 C floats per pixel, DEVICE memory): where each pixel's surface point was one scene update ago
  --  minus where it is (include/art_hip.h ArtMotionSource, 40 bytes, states the arithmetic).  Flat scene: cur_pos3f and prev_pos3f, both or
  --  neither; instanced scene: prev_m12f; Null_Address: nothing moved.  buffers may be null when motion3f is given.
  type Art_Motion_Source is record
    cur_pos3f, prev_pos3f : System.Address;         --  3 C floats per vertex, DEVICE memory
    nverts                : Interfaces.Integer_64;
    prev_m12f             : System.Address;         --  12 C floats per instance, DEVICE memory
    n_instances           : Interfaces.Integer_64;
  end record;
  pragma Convention (C, Art_Motion_Source);
  function art_render_aovs_motion_device (p : access constant Art_Pass_Params; buffers : access constant Art_Aov_Buffers;
                                          src : access constant Art_Motion_Source; motion3f : System.Address;
                                          hip_stream : System.Address) return int;
  pragma Import (C, art_render_aovs_motion_device, "art_render_aovs_motion_device");

  --  Edge-avoiding a-trous denoiser over device planes (include/art_hip.h ArtDenoiseParams, 36 bytes, states the arithmetic): color3f,
  --  albedo3f, normal3f (3 C floats per pixel) and depth (1) are DEVICE memory of the library's GPU, row-major; the three guides may be
  --  Null_Address; out3f may be color3f.  Needs no scene and no viewport; hip_stream = Null_Address is the library's stream.
  type Art_Denoise_Params is record
    width, height : int;
    iterations    : int;     --  1 .. 8
    demodulate    : int;
    normal_log2   : int;     --  0 .. 10
    variant       : int;     --  0 .. 2
    scale         : C_float;
    sigma_color   : C_float;
    sigma_depth   : C_float;
  end record;
  pragma Convention (C, Art_Denoise_Params);

  function art_denoise_device (p : access constant Art_Denoise_Params; color3f, albedo3f, normal3f, depth, out3f : System.Address;
                               hip_stream : System.Address) return int;
  pragma Import (C, art_denoise_device, "art_denoise_device");

  --  The variance-guided variant (include/art_hip.h ArtSvgfParams, 36 bytes): moments2f is the plane of art_bind_moments (2 C floats per
  --  pixel), n_colours the colours behind it; variance_out (1 C float per pixel) may be Null_Address.
  type Art_Svgf_Params is record
    width, height : int;
    iterations    : int;     --  1 .. 8
    demodulate    : int;
    normal_log2   : int;     --  0 .. 10
    n_colours     : int;     --  >= 2
    scale         : C_float;
    sigma_color   : C_float;
    sigma_depth   : C_float;
  end record;
  pragma Convention (C, Art_Svgf_Params);

  function art_denoise_svgf_device (p : access constant Art_Svgf_Params; color3f, moments2f, albedo3f, normal3f, depth, out3f,
                                    variance_out : System.Address; hip_stream : System.Address) return int;
  pragma Import (C, art_denoise_svgf_device, "art_denoise_svgf_device");

  --  The same filter fed by a variance plane (1 C float per pixel, art_temporal_device's variance_out) instead of the moments;
  --  p.n_colours is ignored.
  function art_denoise_svgf_var_device (p : access constant Art_Svgf_Params; color3f, variance1f, albedo3f, normal3f, depth, out3f,
                                        variance_out : System.Address; hip_stream : System.Address) return int;
  pragma Import (C, art_denoise_svgf_var_device, "art_denoise_svgf_var_device");

  --  Temporal reprojection and accumulation (include/art_hip.h ArtTemporalParams, 188 bytes, states the arithmetic): the current frame's
  --  planes, the previous history (Null_Address: the first frame) and the new one, art_temporal_history_bytes (w, h) bytes each, all
  --  DEVICE memory; normal3f, depth, id, out3f, variance_out and length_out may be Null_Address.
  type Art_Temporal_Camera is record
    cam_pos       : Float3_C;
    cam_matrix    : Float16_C;    --  row-major; elements 3, 7 and 11 must be zero
    width, height : int;
  end record;
  pragma Convention (C, Art_Temporal_Camera);
  type Art_Temporal_Params is record
    cur, prev   : Art_Temporal_Camera;
    n_colours   : int;     --  >= 1
    max_history : int;     --  n_colours .. 2 ** 24
    scale       : C_float;
    depth_tol   : C_float;
    normal_min  : C_float;
  end record;
  pragma Convention (C, Art_Temporal_Params);

  function art_temporal_device (p : access constant Art_Temporal_Params; color3f, moments2f, normal3f, depth, id, hist_in, hist_out, out3f,
                                variance_out, length_out : System.Address; hip_stream : System.Address) return int;
  pragma Import (C, art_temporal_device, "art_temporal_device");
  --  art_temporal_device following moved geometry: motion3f is art_render_aovs_motion_device's plane of the current frame
  --  (Null_Address: the call is art_temporal_device).
  function art_temporal_motion_device (p : access constant Art_Temporal_Params; color3f, moments2f, normal3f, depth, id, motion3f, hist_in,
                                       hist_out, out3f, variance_out, length_out : System.Address; hip_stream : System.Address) return int;
  pragma Import (C, art_temporal_motion_device, "art_temporal_motion_device");
  function art_temporal_history_bytes (width, height : int) return long;
  pragma Import (C, art_temporal_history_bytes, "art_temporal_history_bytes");

  --  SVGF's spatial variance estimate (include/art_hip.h ArtSvgfSpatialParams, 24 bytes, states the arithmetic): between
  --  art_temporal_device and art_denoise_svgf_var_device.  hist is art_temporal_device's hist_out; variance_out1f may be variance_in1f
  --  itself and must not overlap hist; all DEVICE memory.
  type Art_Svgf_Spatial_Params is record
    width, height : int;
    radius        : int;     --  1 .. 3; 3 = the 7 x 7 window
    normal_log2   : int;     --  0 .. 10
    min_history   : C_float; --  a pixel with at least this many colours and a finite variance keeps its variance
    sigma_depth   : C_float; --  <= 0: no depth stop
  end record;
  pragma Convention (C, Art_Svgf_Spatial_Params);
  function art_svgf_spatial_variance_device (p : access constant Art_Svgf_Spatial_Params; hist, variance_in1f, variance_out1f : System.Address;
                                             hip_stream : System.Address) return int;
  pragma Import (C, art_svgf_spatial_variance_device, "art_svgf_spatial_variance_device");

  --  The display transform (include/art_hip.h states the arithmetic): an exposure from the histogram of log2 luminance, kept in a state
  --  of art_exposure_state_bytes bytes of DEVICE memory that the caller zeroes once (ArtExposureParams, 44 bytes), and the HDR plane as
  --  8-bit screen words (ArtDisplayParams, 36 bytes).  color3f is row-major DEVICE memory; screen1u and ldr3f are written in `layout`
  --  (ART_LAYOUT_ADA_XY: screen_buffer (x, y) as it is); exposure_state, and one of screen1u and ldr3f, may be Null_Address.
  ART_CURVE_REFERENCE : constant := 0;  ART_CURVE_LINEAR : constant := 1;  ART_CURVE_REINHARD : constant := 2;  ART_CURVE_ACES : constant := 3;
  ART_TRANSFER_SQRT : constant := 0;    ART_TRANSFER_SRGB : constant := 1; ART_TRANSFER_GAMMA22 : constant := 2;
  type Art_Exposure_Params is record
    width, height : int;
    scale         : C_float;  --  the factor on color3f, e.g. 1 / spp
    min_log2, max_log2 : C_float;            --  the histogram's range of log2 luminance; -12 and 4
    low_fraction, high_fraction : C_float;   --  the ranks the mean is taken over; 0.5 and 0.95
    key           : C_float;  --  0.18
    adapt         : C_float;  --  (0, 1]; 1 jumps to the target
    min_exposure, max_exposure : C_float;
  end record;
  pragma Convention (C, Art_Exposure_Params);
  type Art_Display_Params is record
    width, height : int;
    scale         : C_float;
    exposure      : C_float;  --  used when exposure_state is Null_Address
    curve         : int;      --  ART_CURVE_...; ART_CURVE_REFERENCE gives the words of art_download
    transfer      : int;      --  ART_TRANSFER_...
    white         : C_float;  --  ART_CURVE_REINHARD's white point
    dither        : int;      --  0 or 1
    layout        : int;      --  ART_LAYOUT_...
  end record;
  pragma Convention (C, Art_Display_Params);
  function art_exposure_state_bytes return long;
  pragma Import (C, art_exposure_state_bytes, "art_exposure_state_bytes");
  function art_auto_exposure_device (p : access constant Art_Exposure_Params; color3f, state : System.Address;
                                     hip_stream : System.Address) return int;
  pragma Import (C, art_auto_exposure_device, "art_auto_exposure_device");
  function art_display_device (p : access constant Art_Display_Params; color3f, exposure_state, screen1u, ldr3f : System.Address;
                               hip_stream : System.Address) return int;
  pragma Import (C, art_display_device, "art_display_device");

  --  Guided upsampling of a low-resolution render (include/art_hip.h states the arithmetic): lo_color3f at lo_width x lo_height becomes
  --  out3f at width x height under the feature buffers of both resolutions (Art_Upsample_Guides: DEVICE memory, Null_Address = not
  --  given, each plane on both sides or on neither).  fallback1b (one byte per hi pixel, may be Null_Address): 0 guided, 1 unguided, 2 black.
  type Art_Upsample_Jitter is array (0 .. 1) of C_float;
  pragma Convention (C, Art_Upsample_Jitter);
  type Art_Upsample_Params is record
    width, height       : int;      --  the output frame
    lo_width, lo_height : int;      --  the input frame; 1 .. width and 1 .. height
    footprint           : int;      --  2 or 4
    demodulate          : int;      --  1: divide by the lo albedo, multiply by the hi albedo
    normal_log2         : int;      --  0 .. 10
    scale               : C_float;  --  the factor on lo_color3f, e.g. 1 / spp
    sigma_depth         : C_float;  --  <= 0: no depth stop
    jitter              : Art_Upsample_Jitter;  --  sub-pixel offset of the lo samples, each in (-0.5, 0.5)
  end record;
  pragma Convention (C, Art_Upsample_Params);
  type Art_Upsample_Guides is record
    albedo3f, normal3f, depth, id : System.Address;
  end record;
  pragma Convention (C, Art_Upsample_Guides);
  function art_upsample_device (p : access constant Art_Upsample_Params; lo_color3f : System.Address; lo, hi : access constant Art_Upsample_Guides;
                                out3f, fallback1b : System.Address; hip_stream : System.Address) return int;
  pragma Import (C, art_upsample_device, "art_upsample_device");

  --  Temporal super-resolution (include/art_hip.h states the arithmetic): a jittered lo frame (lo_color3f, lo_moments2f at lo_width x
  --  lo_height) is accumulated into a history at t.cur's size; t.cur and t.prev are the UNJITTERED cameras.  Guides: DEVICE memory,
  --  Null_Address = not given, normal / depth / id on both sides or on neither, motion3f on the hi side only.  The histories are
  --  art_temporal_device's.  out3f, variance_out, length_out and fallback1b (0 filled, 1 unguided, 2 zero) may be Null_Address.
  type Art_Temporal_Upsample_Guides is record
    normal3f, depth, id, motion3f : System.Address;
  end record;
  pragma Convention (C, Art_Temporal_Upsample_Guides);
  type Art_Temporal_Upsample_Params is record
    t                   : Art_Temporal_Params;
    lo_width, lo_height : int;
    jitter              : Art_Upsample_Jitter;  --  this frame's offset of the lo samples, each in (-0.5, 0.5)
    radius              : C_float;  --  (0, min (width / lo_width, height / lo_height)], in hi pixels
    min_confidence      : C_float;  --  (0, 1]
  end record;
  pragma Convention (C, Art_Temporal_Upsample_Params);
  function art_temporal_upsample_device (p : access constant Art_Temporal_Upsample_Params; lo_color3f, lo_moments2f : System.Address;
                                         lo, hi : access constant Art_Temporal_Upsample_Guides;
                                         hist_in, hist_out, out3f, variance_out, length_out, fallback1b : System.Address;
                                         hip_stream : System.Address) return int;
  pragma Import (C, art_temporal_upsample_device, "art_temporal_upsample_device");

  --  Firefly suppression ahead of temporal accumulation (include/art_hip.h states the arithmetic): a pixel whose luminance exceeds
  --  gain * (the rank-th largest luminance among its neighbours) + floor is scaled down to that limit, its moments with it.  Planes:
  --  DEVICE memory; moments2f and moments_out2f are both given or both Null_Address; id and clamped1b (0 kept, 1 clamped, 2 not finite)
  --  may be Null_Address.  out3f may be color3f and moments_out2f may be moments2f.  out3f holds the SCALED colour.
  type Art_Firefly_Params is record
    width, height : int;
    radius        : int;      --  1 or 2
    rank          : int;      --  1 .. 4
    min_count     : int;      --  rank .. (2 * radius + 1) ** 2 - 1
    scale         : C_float;  --  the factor on color3f, e.g. 1 / spp
    gain          : C_float;  --  finite, >= 1
    floor         : C_float;  --  finite, >= 0
  end record;
  pragma Convention (C, Art_Firefly_Params);
  function art_firefly_device (p : access constant Art_Firefly_Params; color3f, moments2f, id, out3f, moments_out2f, clamped1b : System.Address;
                               hip_stream : System.Address) return int;
  pragma Import (C, art_firefly_device, "art_firefly_device");

  --  Bloom ahead of the display transform (include/art_hip.h states the arithmetic): the frame is filtered down a pyramid of halved
  --  levels, the levels are blended back up with scatter, and the result B is mixed in: out = s + strength * (B - s).  Planes: DEVICE
  --  memory, three floats per pixel; exposure_state (the state of art_auto_exposure_device) may be Null_Address = the record's
  --  exposure; out3f and bloom3f (B alone) may each be Null_Address, not both; out3f may be color3f.  out3f holds the SCALED colour.
  type Art_Bloom_Params is record
    width, height : int;
    levels        : int;      --  1 .. 8
    karis         : int;      --  0 / 1: the first downsample weights its five boxes by 1 / (1 + luminance)
    variant       : int;      --  0: the small levels in one workgroup; 1: one launch per level; the same words
    scale         : C_float;  --  the factor on color3f, e.g. 1 / spp
    exposure      : C_float;  --  used when exposure_state is Null_Address; only the threshold reads it
    threshold     : C_float;  --  finite, >= 0: the soft threshold on exposure * luminance
    knee          : C_float;  --  finite, >= 0
    scatter       : C_float;  --  0 .. 1
    strength      : C_float;  --  0 .. 1
  end record;
  pragma Convention (C, Art_Bloom_Params);
  function art_bloom_device (p : access constant Art_Bloom_Params; color3f, exposure_state, out3f, bloom3f : System.Address;
                             hip_stream : System.Address) return int;
  pragma Import (C, art_bloom_device, "art_bloom_device");

  --  Adaptive sampling (include/art_hip.h states the contracts and the arithmetic).  mask1b: one byte per pixel of the frame, row-major,
  --  DEVICE memory, non-zero = selected.  art_compact_mask_device: the selected pixels of this rank's list, in list order, into pixels_out
  --  (cap words, DEVICE memory) and their number into count_out (one DEVICE word).
  function art_compact_mask_device (mask1b, pixels_out : System.Address; cap : long; count_out : System.Address;
                                    hip_stream : System.Address) return int;
  pragma Import (C, art_compact_mask_device, "art_compact_mask_device");
  --  One Render_Pass over the selected pixels only; spp advances by the pass's samples whatever the mask holds.  counts1u (DEVICE, one
  --  32-bit word per pixel, may be Null_Address) receives the samples added; pixels_out (host, may be null) the pixels rendered.
  --  The host waits once for the list's length, and at the end as art_render_pass does.
  function art_render_pass_masked (p : access constant Art_Pass_Params; mask1b, counts1u : System.Address; spp_inout : access int;
                                   pixels_out : access long) return int;
  pragma Import (C, art_render_pass_masked, "art_render_pass_masked");
  --  Radiance along the caller's rays (include/art_hip.h states the contract): `samples` paths per ray with the integrator render_type
  --  selects, added into radiance3f (and moments2f, may be Null_Address).  All arrays are DEVICE memory; keys1u may be Null_Address
  --  (ray i has RNG key i).  Runs on the library's stream and waits at the end, as art_render_pass_masked does (ArtRadianceParams, 24 bytes).
  type Art_Radiance_Params is record
    render_type : int;          --  ART_PT_STUPID | ART_PT_SHADOW | ART_PT_MIS
    max_depth   : int;          --  1 .. 16
    samples     : int;          --  >= 1
    sample_base : Unsigned_32;
    seed        : Unsigned_64;
  end record;
  pragma Convention (C, Art_Radiance_Params);
  function art_radiance_rays_device (p : access constant Art_Radiance_Params; origins3f, dirs3f, keys1u : System.Address;
                                     n : Interfaces.Integer_64; radiance3f, moments2f : System.Address) return int;
  pragma Import (C, art_radiance_rays_device, "art_radiance_rays_device");
  --  Per pixel: mean colour, variance of the mean's luminance, relative error and the next mask (ArtAdaptiveParams, 28 bytes).  The four
  --  outputs may each be Null_Address, but not all.
  type Art_Adaptive_Params is record
    width, height : int;
    aa_on         : int;
    min_colours   : int;     --  >= 2
    max_samples   : int;     --  >= 0
    threshold     : C_float;
    lum_floor     : C_float; --  >= 0
  end record;
  pragma Convention (C, Art_Adaptive_Params);
  function art_adaptive_estimate_device (p : access constant Art_Adaptive_Params; accum3f, moments2f, counts1u, mean3f, variance1f, error1f,
                                         mask1b : System.Address; hip_stream : System.Address) return int;
  pragma Import (C, art_adaptive_estimate_device, "art_adaptive_estimate_device");

  --  Luminance moments of the render passes in caller-owned DEVICE memory: 2 C floats {S1, S2} per pixel, row-major, zeroed by
  --  art_resize, added to by every art_render_pass (include/art_hip.h).  Null_Address: none (the default).
  --  The camera of the uploaded scene, without a rebuild (include/art_hip.h): stream-ordered on the library's stream, every context.
  function art_set_camera (cam_pos : access constant Float3_C; cam_matrix : access constant Float16_C) return int;
  pragma Import (C, art_set_camera, "art_set_camera");

  function art_bind_moments (device_moments_rowmajor : System.Address) return int;
  pragma Import (C, art_bind_moments, "art_bind_moments");

  --  Deforming mesh number `mesh` (an index into Art_Scene_Desc.meshes) of an uploaded instanced scene: pos3f / nrm3f are DEVICE memory
  --  of the library's GPU, 3 * nverts C floats in the vertex order of that mesh, object space; nrm3f = Null_Address keeps the normals;
  --  hip_stream = Null_Address is the library's stream.  Stream-ordered; the picture is the one of art_upload_scene with that mesh's
  --  vertices replaced, at the matrices in force (include/art_hip.h).
  function art_refit_mesh_device (mesh : int; pos3f, nrm3f : System.Address; nverts : Interfaces.Integer_64;
                                  hip_stream : System.Address) return int;
  pragma Import (C, art_refit_mesh_device, "art_refit_mesh_device");

  type Art_Mesh_Refit_Info is record   --  include/art_hip.h ArtMeshRefitInfo, 40 bytes; cumulative since art_upload_scene
    refits       : Unsigned_64;
    refit_ms     : double;
    plan_ms      : double;
    bad_vertices : Unsigned_64;
    repads       : Unsigned_64;
  end record;
  pragma Convention (C, Art_Mesh_Refit_Info);

  function art_get_mesh_refit_info (info : access Art_Mesh_Refit_Info) return int;   --  waits for the refits enqueued so far
  pragma Import (C, art_get_mesh_refit_info, "art_get_mesh_refit_info");

  --  A new tree for mesh number `mesh` of an uploaded instanced scene, built on the GPU from that mesh's triangle records as the last
  --  art_refit_mesh_device left them; returns when the tree is committed (include/art_hip.h).  art_get_mesh_tree_cost (include/art_hip.h)
  --  has the figure to decide when.
  function art_rebuild_mesh_tree_device (mesh : int; hip_stream : System.Address) return int;
  pragma Import (C, art_rebuild_mesh_tree_device, "art_rebuild_mesh_tree_device");

  type Art_Mesh_Rebuild_Info is record   --  include/art_hip.h ArtMeshRebuildInfo, 32 bytes; cumulative since art_upload_scene
    rebuilds  : Unsigned_64;
    gather_ms : double;
    build_ms  : double;
    host_ms   : double;
  end record;
  pragma Convention (C, Art_Mesh_Rebuild_Info);

  function art_get_mesh_rebuild_info (info : access Art_Mesh_Rebuild_Info) return int;
  pragma Import (C, art_get_mesh_rebuild_info, "art_get_mesh_rebuild_info");

  type Art_Tree_Cost is record   --  include/art_hip.h ArtTreeCost, 32 bytes
    root_area, node_visits, leaf_visits, tri_tests : double;
  end record;
  pragma Convention (C, Art_Tree_Cost);

  function art_get_mesh_tree_cost (mesh : int; cost : access Art_Tree_Cost) return int;   --  device 0; waits for the library's stream
  pragma Import (C, art_get_mesh_tree_cost, "art_get_mesh_tree_cost");

  function art_last_error return Interfaces.C.Strings.chars_ptr;
  pragma Import (C, art_last_error, "art_last_error");

  procedure art_shutdown;
  pragma Import (C, art_shutdown, "art_shutdown");

end Art_Hip;
