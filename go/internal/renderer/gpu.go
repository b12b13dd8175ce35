//go:build rtgo

// gpu.go — the cgo shim that puts the reference's Render path on MI355X GPUs.
//
// Drop this file into raytraceGo's internal/renderer (the package of
// renderer.go) and build with `go build -tags rtgo`; set
//     CGO_CFLAGS="-I<this repo>/include"
//     CGO_LDFLAGS="-L<this repo>/concurrent-raytracer-go_amd/build -Wl,-rpath,<same>"
// so cgo finds rt_api.h and librtgo.so (make -C concurrent-raytracer-go_amd).
// RenderSequenceGPU allocates device images itself, so the file also includes
// hip_runtime_api.h and links libamdhip64: add -I<rocm>/include and
// -L<rocm>/lib to the two variables.
// RenderGPU has Render's signature and meaning (renderer.go:67-126): it
// returns a new *image.RGBA whose row y is Go image row y, tone-mapped by
// toneMap + ToRGB (renderer.go:348-367, vector.go:106-109), and fills the
// same benchmarkData fields (renderer.go:103-112).  cmd/raytracer/main.go:49
// calls it in place of Render (INTEGRATION.md §1).
//
// The scene crosses the boundary as the JSON it was loaded from:
// json.Marshal of *scene.Scene (Vec3.MarshalJSON writes [x, y, z],
// vector.go:195-197) parsed by rt_scene_parse_json, which applies
// createMaterial's defaults and GetHittables' type rules (scene.go:59-148)
// exactly as the C++ loader does for a file.  One rt_renderer per
// ParallelRenderer holds the devices' scenes, schedules and buffers between
// calls (NewParallelRenderer once, Render per frame); RT_DEVICES sets how many
// GPUs it shards the tiles over (default 1), RT_CAMERA=lookat opts in to the
// scene's own camera orientation and field of view (rt_settings.camera).
//
// RenderSequenceGPU (DESIGN.md §4.11) renders the scene from several cameras
// -- a turntable, a fly-through -- as camera sequences of at most RT_MAX_FRAMES
// frames per launch, through an rt_context of its own and the two entry points
//     int rt_context_render_cameras_async(rt_context* ctx, int32_t width, int32_t height,
//         const rt_settings* settings, int32_t nframes, const rt_camera* cameras, const uint64_t* seeds,
//         int32_t rank, int32_t world, int32_t layout, float* const* d_linear, uint8_t* const* d_rgba,
//         void* hip_stream);
//     int rt_camera_orbit(const rt_camera* cam, int32_t n, double degrees, rt_camera* out);
// OrbitCameras is rt_camera_orbit on scene.Camera values.
//
// Go cannot run in the image this was written in (no toolchain, SURVEY.md
// §8c): tests/c/shim_sequence.c makes exactly this file's C call sequence
// and is run by the test suite instead.
package renderer

/*
#cgo CFLAGS: -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -lrtgo -lamdhip64
#include <stdlib.h>
#include <hip/hip_runtime_api.h>
#include "rt_api.h"
*/
import "C"

import (
	"encoding/json"
	"fmt"
	"image"
	"os"
	"strconv"
	"sync"
	"time"
	"unsafe"

	"raytraceGo/internal/scene"
)

var (
	gpuMu        sync.Mutex
	gpuRenderers = map[*ParallelRenderer]*C.rt_renderer{}
)

func cbool(b bool) C.int32_t {
	if b {
		return 1
	}
	return 0
}

func rtError(what string, rc C.int) error {
	return fmt.Errorf("%s failed (%d): %s", what, int(rc), C.GoString(C.rt_last_error()))
}

// gpuRenderer returns r's rt_renderer, made on first use (rt_renderer_create).
func (r *ParallelRenderer) gpuRenderer() (*C.rt_renderer, error) {
	gpuMu.Lock()
	defer gpuMu.Unlock()
	if h, ok := gpuRenderers[r]; ok {
		return h, nil
	}
	n := 1
	if v, err := strconv.Atoi(os.Getenv("RT_DEVICES")); err == nil && v > 0 {
		n = v
	}
	var h *C.rt_renderer
	if rc := C.rt_renderer_create(nil, C.int32_t(n), &h); rc != C.RT_OK {
		return nil, rtError("rt_renderer_create", rc)
	}
	gpuRenderers[r] = h
	return h, nil
}

// StartGPU makes r's rt_renderer now (HIP runtime start-up, contexts, the
// kernels' code objects): the devices' constructor work, so that a caller
// that times Render after NewParallelRenderer (cmd/raytracer/main.go:46-51,
// renderer.go:68,101) keeps it out of the timed call.  RenderGPU makes the
// renderer itself when StartGPU has not run.
func (r *ParallelRenderer) StartGPU() error {
	_, err := r.gpuRenderer()
	return err
}

// CloseGPU frees r's devices' resources (rt_renderer_destroy).
func (r *ParallelRenderer) CloseGPU() {
	gpuMu.Lock()
	defer gpuMu.Unlock()
	if h, ok := gpuRenderers[r]; ok {
		C.rt_renderer_destroy(h)
		delete(gpuRenderers, r)
	}
}

// RenderGPU is Render (renderer.go:67-126) on the GPUs.  Like Render it has
// no error return: a failure of the device path panics with the library's
// message (the reference panics on bad scene input, scene.go:113).
func (r *ParallelRenderer) RenderGPU(s *scene.Scene, width, height int) *image.RGBA {
	start := time.Now()
	data, err := json.Marshal(s)
	if err != nil {
		panic(fmt.Sprintf("RenderGPU: %v", err))
	}
	cdata := C.CBytes(data)
	defer C.free(cdata)
	var sb *C.rt_scene_buf
	// verbose 1: the lines Render prints through GetHittables (scene.go:62-88)
	if rc := C.rt_scene_parse_json((*C.char)(cdata), C.size_t(len(data)), 1, &sb); rc != C.RT_OK {
		panic(rtError("rt_scene_parse_json", rc).Error())
	}
	defer C.rt_scene_free(sb)

	var st C.rt_settings // settings.go:3-25 through the renderer's fields
	C.rt_settings_default(&st)
	st.samples = C.int32_t(r.samples)
	st.max_depth = C.int32_t(r.maxDepth)
	st.anti_aliasing = cbool(r.antiAliasing)
	st.recursive_reflections = cbool(r.recursiveReflections)
	st.soft_shadows = cbool(r.softShadows)
	st.depth_of_field = cbool(r.depthOfField)
	st.num_workers = C.int32_t(r.numWorkers)
	// getRay's fixed -Z view (renderer.go:377-390) unless RT_CAMERA=lookat opts
	// in to the scene's own lookAt / up / fov (rt_api.h RT_CAMERA_*)
	st.camera = C.RT_CAMERA_REFERENCE
	if os.Getenv("RT_CAMERA") == "lookat" {
		st.camera = C.RT_CAMERA_LOOKAT
	}

	img := image.NewRGBA(image.Rect(0, 0, width, height))
	var stats C.rt_stats
	if width <= 0 || height <= 0 {
		// Render with no tiles (createRenderTasks makes none): an empty image
		stats.objects = C.int32_t(C.rt_scene_view(sb).num_objects)
		stats.lights = C.int32_t(C.rt_scene_view(sb).num_lights)
		return r.finishGPU(s, img, width, height, start, stats)
	}
	h, err := r.gpuRenderer()
	if err != nil {
		panic(err.Error())
	}
	// img.Pix: W*H*4 bytes, row y = Go image row y, the layout rt_renderer_render
	// writes; a Go pointer to pointer-free memory, not retained (cgo rules)
	rc := C.rt_renderer_render(h, C.rt_scene_view(sb), C.int32_t(width), C.int32_t(height), &st, nil,
		(*C.uint8_t)(unsafe.Pointer(&img.Pix[0])), &stats)
	if rc != C.RT_OK {
		panic(rtError("rt_renderer_render", rc).Error())
	}
	return r.finishGPU(s, img, width, height, start, stats)
}

// finishGPU records Render's benchmark data and prints its closing lines
// (renderer.go:101-123).
func (r *ParallelRenderer) finishGPU(s *scene.Scene, img *image.RGBA, width, height int, start time.Time,
	stats C.rt_stats) *image.RGBA {
	renderTime := time.Since(start)
	r.benchmarkData.SceneName = s.GetSceneName() // renderer.go:103-112
	r.benchmarkData.Resolution = fmt.Sprintf("%dx%d", width, height)
	r.benchmarkData.RenderTime = renderTime.Seconds()
	r.benchmarkData.Samples = r.samples
	r.benchmarkData.MaxDepth = r.maxDepth
	r.benchmarkData.NumWorkers = r.numWorkers
	r.benchmarkData.Objects = int(stats.objects)
	r.benchmarkData.Lights = int(stats.lights)
	r.benchmarkData.Timestamp = time.Now()
	r.benchmarkData.Features = []string{
		"Improved metallic reflections with Fresnel effect",
		"Shiny materials with configurable roughness and specular",
		"Enhanced light source reflections",
		"Better specular highlights for metallic surfaces",
	}
	fmt.Printf("Rendering complete!\n")
	fmt.Printf("Enhanced materials features:\n")
	for _, feature := range r.benchmarkData.Features {
		fmt.Printf("- %s\n", feature)
	}
	return img
}

// cCamera is c as an rt_camera (scene.go:18-24).
func cCamera(c scene.Camera) C.rt_camera {
	var o C.rt_camera
	o.position = [3]C.double{C.double(c.Position.X), C.double(c.Position.Y), C.double(c.Position.Z)}
	o.look_at = [3]C.double{C.double(c.LookAt.X), C.double(c.LookAt.Y), C.double(c.LookAt.Z)}
	o.up = [3]C.double{C.double(c.Up.X), C.double(c.Up.Y), C.double(c.Up.Z)}
	o.fov = C.double(c.FOV)
	o.aspect_ratio = C.double(c.AspectRatio)
	return o
}

// OrbitCameras returns n views on a circle around cam's LookAt, about its Up
// axis, `degrees` in all (rt_camera_orbit: view k is turned by degrees*k/n and
// view 0 is cam itself).
func OrbitCameras(cam scene.Camera, n int, degrees float64) ([]scene.Camera, error) {
	if n < 1 {
		return nil, fmt.Errorf("OrbitCameras: n must be >= 1")
	}
	in := cCamera(cam)
	out := make([]C.rt_camera, n)
	if rc := C.rt_camera_orbit(&in, C.int32_t(n), C.double(degrees), &out[0]); rc != C.RT_OK {
		return nil, rtError("rt_camera_orbit", rc)
	}
	views := make([]scene.Camera, n)
	for k := range views {
		views[k] = cam
		views[k].Position.X = float64(out[k].position[0])
		views[k].Position.Y = float64(out[k].position[1])
		views[k].Position.Z = float64(out[k].position[2])
	}
	return views, nil
}

// RenderSequenceGPU renders s once per camera of cams: image f is what
// RenderGPU returns for s with its Camera replaced by cams[f].  The frames of
// a launch share one work schedule and, for scenes of spheres alone, one
// streamed kernel launch (rt_context_render_cameras_async); other scenes
// render frame by frame behind the same call.  One device, a context made and
// freed by the call.  Like RenderGPU it panics on a library failure.
func (r *ParallelRenderer) RenderSequenceGPU(s *scene.Scene, width, height int, cams []scene.Camera) []*image.RGBA {
	if len(cams) == 0 || width <= 0 || height <= 0 {
		return nil
	}
	data, err := json.Marshal(s)
	if err != nil {
		panic(fmt.Sprintf("RenderSequenceGPU: %v", err))
	}
	cdata := C.CBytes(data)
	defer C.free(cdata)
	var sb *C.rt_scene_buf
	if rc := C.rt_scene_parse_json((*C.char)(cdata), C.size_t(len(data)), 0, &sb); rc != C.RT_OK {
		panic(rtError("rt_scene_parse_json", rc).Error())
	}
	defer C.rt_scene_free(sb)
	var st C.rt_settings
	C.rt_settings_default(&st)
	st.samples = C.int32_t(r.samples)
	st.max_depth = C.int32_t(r.maxDepth)
	st.recursive_reflections = cbool(r.recursiveReflections)
	st.soft_shadows = cbool(r.softShadows)
	st.camera = C.RT_CAMERA_REFERENCE
	if os.Getenv("RT_CAMERA") == "lookat" {
		st.camera = C.RT_CAMERA_LOOKAT
	}
	var ctx *C.rt_context
	if rc := C.rt_context_create(0, &ctx); rc != C.RT_OK {
		panic(rtError("rt_context_create", rc).Error())
	}
	defer C.rt_context_destroy(ctx)
	if rc := C.rt_context_set_scene(ctx, C.rt_scene_view(sb), 0); rc != C.RT_OK {
		panic(rtError("rt_context_set_scene", rc).Error())
	}
	npix := C.size_t(width) * C.size_t(height)
	per := len(cams)
	if per > C.RT_MAX_FRAMES {
		per = C.RT_MAX_FRAMES
	}
	// device images of one launch: float3 linear (required) and RGBA8 per frame
	var dLin, dImg unsafe.Pointer
	if C.hipMalloc(&dLin, C.size_t(per)*npix*12) != C.hipSuccess || C.hipMalloc(&dImg, C.size_t(per)*npix*4) != C.hipSuccess {
		panic("RenderSequenceGPU: hipMalloc failed")
	}
	defer C.hipFree(dLin)
	defer C.hipFree(dImg)
	// (pointer tables in C memory: cgo forbids passing Go memory that holds pointers)
	lin := (*[C.RT_MAX_FRAMES]*C.float)(C.malloc(C.size_t(C.RT_MAX_FRAMES) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	img := (*[C.RT_MAX_FRAMES]*C.uint8_t)(C.malloc(C.size_t(C.RT_MAX_FRAMES) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(lin))
	defer C.free(unsafe.Pointer(img))
	for f := 0; f < per; f++ {
		lin[f] = (*C.float)(unsafe.Add(dLin, uintptr(f)*uintptr(npix)*12))
		img[f] = (*C.uint8_t)(unsafe.Add(dImg, uintptr(f)*uintptr(npix)*4))
	}
	out := make([]*image.RGBA, len(cams))
	ccams := make([]C.rt_camera, per)
	for f0 := 0; f0 < len(cams); f0 += per {
		m := len(cams) - f0
		if m > per {
			m = per
		}
		for f := 0; f < m; f++ {
			ccams[f] = cCamera(cams[f0+f])
		}
		rc := C.rt_context_render_cameras_async(ctx, C.int32_t(width), C.int32_t(height), &st, C.int32_t(m), &ccams[0], nil,
			0, 1, C.RT_LAYOUT_IMAGE, &lin[0], &img[0], nil)
		if rc != C.RT_OK {
			panic(rtError("rt_context_render_cameras_async", rc).Error())
		}
		for f := 0; f < m; f++ { // (hipMemcpy waits for the launch on the default stream)
			out[f0+f] = image.NewRGBA(image.Rect(0, 0, width, height))
			if C.hipMemcpy(unsafe.Pointer(&out[f0+f].Pix[0]), unsafe.Pointer(img[f]), npix*4, C.hipMemcpyDeviceToHost) != C.hipSuccess {
				panic("RenderSequenceGPU: hipMemcpy failed")
			}
		}
	}
	return out
}
