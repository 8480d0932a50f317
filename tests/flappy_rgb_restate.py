"""NumPy restatement of the Flappy env's COLOUR rendering (rltime_amd/acting/flappy_env.py rgb=True; csrc/acting.hip
k_flappy_env_step with FlappyArgs.rgb), beside tests/flappy_restate.py, whose game it is: dynamics, record, Philox keying,
rewards and dones are that module's, untouched.  Only the observation differs:

  observation      ONE frame, the current state's (history depth 1 — nothing predates the episode, so the reset frame is drawn
                   like any other), as three planes (red, green, blue) of H x W uint8: every pixel is the background colour
                   (78, 192, 202), except the cells of every on-screen pipe's column outside its gap, which are (84, 168, 40),
                   and the bird's cell (rows[0], column 1), which is (250, 200, 30) and drawn last.

Proved on hand-built frames by tests/test_flappy_rgb_cpu.py; the kernel is held to it bit for bit by
tests/test_flappy_rgb_gpu.py.  `to_classes` maps a colour frame back through the palette, which is how the colour env is
tied to the intensity env's frames (tests/flappy_restate.py BIRD / PIPE / 0)."""
import numpy as np

from tests.flappy_restate import BIRD, BIRD_COLUMN, PIPE, gap_top, pipes_on_screen

BACKGROUND_RGB, PIPE_RGB, BIRD_RGB = (78, 192, 202), (84, 168, 40), (250, 200, 30)


def render_rgb(state, seed, H, W, s, g, D):
    """-> frames (E, 3, H, W) uint8 of `state` (tests/flappy_restate.py's state dict)."""
    E, R, C = len(state["v"]), H // s, W // s
    frames = np.empty((E, 3, H, W), dtype=np.uint8)
    for e in range(E):
        tau, n = int(state["tau"][e]), int(state["n"][e])
        for p in range(3):
            frames[e, p] = BACKGROUND_RGB[p]
        for j, col in pipes_on_screen(tau, C, D):
            top = gap_top(seed, e, n, j, R, g)
            for p in range(3):
                frames[e, p, :top * s, col * s:(col + 1) * s] = PIPE_RGB[p]
                frames[e, p, (top + g) * s:, col * s:(col + 1) * s] = PIPE_RGB[p]
        y = int(state["rows"][e, 0])
        for p in range(3):
            frames[e, p, y * s:(y + 1) * s, BIRD_COLUMN * s:(BIRD_COLUMN + 1) * s] = BIRD_RGB[p]
    return frames


def to_classes(frames):
    """(E, 3, H, W) colour frames -> (E, 1, H, W) in the intensity env's values (bird 255, pipe 128, background 0); a pixel
    that is none of the three colours is an error."""
    f = np.asarray(frames)
    out = np.full((f.shape[0], 1) + f.shape[2:], 7, dtype=np.uint8)
    for colour, value in ((BACKGROUND_RGB, 0), (PIPE_RGB, PIPE), (BIRD_RGB, BIRD)):
        hit = (f[:, 0] == colour[0]) & (f[:, 1] == colour[1]) & (f[:, 2] == colour[2])
        out[:, 0][hit] = value
    assert not (out == 7).any(), "a pixel off the palette"
    return out
