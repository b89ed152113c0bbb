"""Python recipes of the reference's procedural ray-tracer scenes (DemoScenes, src/raytracer/RTapp_utils.cuh:249-550),
built through ptrt_amd.rt.Scene; each fills the Scene it is given, in the reference's order of calls.  Scalars the
reference computes in float (positions, hues) are computed in float32 here."""
import numpy as np

f32 = np.float32
TWO_PI = f32(6.28318530717958647692)


def _rt():
    import ptrt_amd.rt as rt
    return rt


def _mat(albedo, rough, metal, **kw):
    m = _rt().Material(albedo, rough, metal)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _cube(s, mat):
    return s.mesh(s.addCube(mat))


def cornell(s):
    """createCornellBox (RTapp_utils.cuh:251-312): seven scaled cubes, two rotated boxes, one point light, ambient
    0.02, the sky off."""
    white = _mat((0.73, 0.73, 0.73), 0.6, 0.0, specular=0.04)
    red = _mat((0.65, 0.05, 0.05), 0.6, 0.0, specular=0.04)
    green = _mat((0.12, 0.45, 0.15), 0.6, 0.0, specular=0.04)
    light = _mat((0.0, 0.0, 0.0), 0.0, 0.0, emission=15.0)
    box = _mat((0.9, 0.9, 0.9), 0.2, 0.0, specular=0.04)
    for mat, sc, at in ((white, (10, 10, 0.1), (0, 0, -10)), (red, (0.1, 10, 10), (-5, 0, -5)),
                        (green, (0.1, 10, 10), (5, 0, -5)), (white, (10, 0.1, 10), (0, -5, -5)),
                        (white, (10, 0.1, 10), (0, 5, -5)), (light, (2, 0.1, 2), (0, 4.9, -5))):
        _cube(s, mat).scale(sc).moveTo(at)
    _cube(s, box).scale((1.5, 3.0, 1.5)).moveTo((-1.5, -3.5, -6)).rotateSelfEulerXYZ((0, 0.3, 0))
    _cube(s, box).scale((1.5, 1.5, 1.5)).moveTo((1.5, -4.25, -4)).rotateSelfEulerXYZ((0, -0.4, 0))
    s.addPointLight((0, 4.5, -5), (1.0, 0.9, 0.8), 3.0, 20.0)
    s.setAmbientLight((0.02, 0.02, 0.02))
    s.setCamera((0, 0, 5), (0, 0, -5), (0, 1, 0), 40.0)
    s.disableSky()
    return s


def showcase1(s):
    """createMaterialShowcase1 (RTapp_utils.cuh:314-350): a 3 x 5 grid of cubes, metallic across, roughness up, three
    point lights, a floor plane."""
    rows, cols, spacing = 3, 5, f32(2.5)
    for i in range(rows):
        for j in range(cols):
            metal = f32(j) / f32(cols - 1)
            rough = f32(i) / f32(rows - 1)
            x = (f32(j) - f32(cols / 2.0)) * spacing
            y = (f32(i) - f32(rows / 2.0)) * spacing
            _cube(s, _mat((0.8, 0.3, 0.2), rough, metal, specular=0.04)).scale(0.8).moveTo((x, y, -10))
    s.addPointLight((10, 10, 0), (1.0, 0.95, 0.9), 3.0, 50.0)
    s.addPointLight((-10, 5, 5), (0.4, 0.4, 0.5), 2.0, 40.0)
    s.addPointLight((0, 15, -15), (0.8, 0.8, 1.0), 1.5, 40.0)
    s.setAmbientLight((0.03, 0.03, 0.03))
    s.setCamera((0, 0, 5), (0, 0, -10), (0, 1, 0), 45.0)
    s.addPlaneXZ(-10.0, 50.0, _mat((0.8, 0.8, 0.8), 0.4, 0.0, specular=0.04))
    return s


def light_show(s):
    """createLightShow (RTapp_utils.cuh:352-395): a Water cube in a ring of twelve rotated coloured cubes, four point
    lights and a spot light, a floor plane."""
    rt = _rt()
    _cube(s, rt.Materials.Water()).scale(2.0).moveTo((0, 0, -10))
    n, radius = 12, f32(6.0)
    for i in range(n):
        angle = (TWO_PI * f32(i)) / f32(n)
        hue = f32(i) / f32(n)
        third = TWO_PI / f32(3)
        colour = (f32(0.5) + f32(0.5) * np.cos(TWO_PI * hue), f32(0.5) + f32(0.5) * np.cos(TWO_PI * hue + third),
                  f32(0.5) + f32(0.5) * np.cos(TWO_PI * hue + f32(2) * TWO_PI / f32(3)))
        m = _mat(colour, 0.25, 0.8 if i % 2 else 0.2, specular=0.04)
        at = (radius * np.cos(angle), f32(2.0) * np.sin(angle * f32(2)), f32(-10) + radius * np.sin(angle))
        _cube(s, m).scale(0.7).moveTo(at).rotateSelfEulerXYZ((angle, angle * f32(0.5), 0))
    s.addPointLight((5, 3, -5), (1.0, 0.2, 0.2), 3.0, 30.0)
    s.addPointLight((-5, 3, -5), (0.2, 1.0, 0.2), 3.0, 30.0)
    s.addPointLight((0, -3, -5), (0.2, 0.2, 1.0), 3.0, 30.0)
    s.addPointLight((0, 8, -10), (1.0, 1.0, 1.0), 2.0, 40.0)
    s.addSpotLight((0, 10, 0), (0, -1, -0.5), (1.0, 0.9, 0.7), 4.0, 0.2, 0.4, 30.0)
    s.setAmbientLight((0.01, 0.01, 0.01))
    s.setCamera((8, 5, 8), (0, 0, -10), (0, 1, 0), 50.0)
    s.addPlaneXZ(-5.0, 50.0, _mat((0.8, 0.8, 0.8), 0.4, 0.0, specular=0.04))
    return s


def architectural(s):
    """createArchitectural (RTapp_utils.cuh:397-447): concrete pillars, four glass panels, wooden floor, concrete
    ceiling, a directional and three point lights, a ground plane."""
    concrete = _mat((0.7, 0.7, 0.65), 0.6, 0.0, specular=0.04)
    glass = _mat((0.98, 0.98, 0.98), 0.02, 0.0, specular=0.04, transmission=0.98, ior=1.5)
    wood = _mat((0.55, 0.35, 0.2), 0.45, 0.0, specular=0.04)
    for i in range(5):
        _cube(s, concrete).scale((0.5, 8.0, 0.5)).moveTo((f32(-8.0) + f32(i) * f32(4.0), 0.0, -15.0))
    for i in range(4):
        _cube(s, glass).scale((3.8, 6.0, 0.1)).moveTo((f32(-6.0) + f32(i) * f32(4.0), 0.0, -14.5))
    _cube(s, wood).scale((20.0, 0.2, 20.0)).moveTo((0, -4, -15))
    _cube(s, concrete).scale((20.0, 0.5, 20.0)).moveTo((0, 4, -15))
    s.addDirectionalLight((-0.3, -0.6, -0.5), (1.0, 0.95, 0.8), 1.5)
    for i in range(3):
        s.addPointLight((f32(-4.0) + f32(i) * f32(4.0), 3, -12.0), (1.0, 0.9, 0.7), 0.8, 15.0)
    s.setAmbientLight((0.15, 0.15, 0.2))
    s.setCamera((10, 2, 0), (0, 0, -15), (0, 1, 0), 60.0)
    s.addPlaneXZ(-10.0, 50.0, _mat((0.8, 0.8, 0.8), 0.4, 0.0, specular=0.04))
    return s


def material_showcase(s):
    """createMaterialShowcase (RTapp_utils.cuh:449-548): twenty presets on a 5 x 4 grid of cubes, three point lights,
    a clear-coated floor, a dark sky."""
    M = _rt().Materials
    grid = [[M.Gold(), M.Silver(), M.Copper(), M.BrushedAluminum(), M.OilSlick()],
            [M.Glass(), M.FrostedGlass(), M.Diamond(), M.SoapBubble(), M.Water()],
            [M.CarPaint((0.8, 0.1, 0.1)), M.PearlescentPaint((0.9, 0.9, 1.0)), M.Skin(), M.Jade(), M.Wax()],
            [M.Velvet((0.5, 0.1, 0.6)), M.Silk((0.1, 0.3, 0.8)), M.PlasticRed(), M.RubberBlack(), M.NeonLight((0.3, 0.8, 1.0))]]
    spacing = f32(2.5)
    start_x = -(f32(5 - 1) * spacing) / f32(2.0)
    for row, mats in enumerate(grid):
        for col, mat in enumerate(mats):
            z = f32(-10.0) - f32(row) * spacing if row else f32(-10.0)
            _cube(s, mat).moveTo((start_x + f32(col) * spacing, 0, z)).scale(0.8)
    s.addPointLight((0, 8, -8), (1.0, 1.0, 1.0), 3.0, 50.0)
    s.addPointLight((-8, 4, -4), (1.0, 0.9, 0.8), 2.0, 30.0)
    s.addPointLight((8, 4, -12), (0.8, 0.9, 1.0), 2.0, 30.0)
    s.setAmbientLight((0.03, 0.03, 0.03))
    s.addPlaneXZ(-1.5, 50.0, _mat((0.9, 0.9, 0.9), 0.05, 0.0, specular=0.04, clearcoat=0.5, clearcoat_roughness=0.1))
    s.setCamera((0, 6, 5), (0, -0.5, -10), (0, 1, 0), 45.0)
    s.setSkyGradient((0.05, 0.05, 0.08), (0.02, 0.02, 0.03))
    return s


DEMO_SCENES = {"cornell": cornell, "showcase1": showcase1, "light_show": light_show, "architectural": architectural,
               "material_showcase": material_showcase}


def readme(s):
    """A stand-in of this project's own (the reference documents no ray-tracer example): a ground plane, a glass
    sphere and a point light."""
    rt = _rt()
    s.addPlaneXZ(-1.0, 10.0, rt.Material((0.8, 0.8, 0.8)))
    i = s.addSphere(32, rt.Materials.Glass())
    s.mesh(i).setPosition((0.0, 0.0, -3.0))
    s.addPointLight((2.0, 4.0, -1.0), (1.0, 1.0, 1.0), 2.0)
    s.setCamera((0, 1, 3), (0, 0, -3), (0, 1, 0), 45.0)
    return s
