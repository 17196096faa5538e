"""numpy restatement of the fleet loop's sensor-delay launch (include/duck_fleet.h: duck_fleet_sensor_delay) --
duck_fleet_sense_delay's IMU rule, then the same three-slot delay line for the joint-encoder columns of the
observation, with the encoder delay drawn from word 0 of block 1 of the latency's stream.

The draw is uint32 / uint64 integer arithmetic and the lines copy words (as int32 views: NaN payloads and -0 keep
their bits), so the kernel's outputs equal these bit for bit. The integer map, the clamp, the period and the IMU
part are tests/fleet_latency_reference.py's, imported and not restated. Test infrastructure only.
"""

import numpy as np

from tests.fleet_latency_reference import LAT_SIZE, LAT_TAG, MAX_DELAY, SLOTS, clamp_rows, draw_map, period, sense_delay
from tests.fleet_reference import M32, derive_key
from tests.mlp_reference import threefry2x32

f32 = np.float32
ENC_SIZE = 2          # DUCK_FLEET_ENC_SIZE
ENC_COL = 13          # the first encoder column of an obs row: gyro 3, accelerometer 3, command 7 before it


def clamp_enc(enc):
    """The kernel's clamp of an encoder row, by clamp_rows' rule for a pair: [N][2] int64."""
    enc = np.asarray(enc, dtype=np.int64).reshape(-1, ENC_SIZE)
    return clamp_rows(np.concatenate([enc, np.zeros_like(enc)], axis=1))[:, :ENC_SIZE]


def encoder_delay(seed, robot_offset, lat_tick, enc, tag=LAT_TAG):
    """The encoder delay [N] of the period ``lat_tick`` counts: word 0 of block 1 at counter (p, 1) through the
    integer map of (enc_lo, enc_hi); lo == hi is that value."""
    enc = clamp_enc(enc)
    n = len(enc)
    p = period(lat_tick)
    k0, k1 = derive_key(seed, int(robot_offset) + np.arange(n, dtype=np.int64), tag)
    w0, _ = threefry2x32(k0, k1, p.astype(np.uint64) & np.uint64(M32), np.ones(n, np.uint64))
    return draw_map(w0, enc[:, 0], enc[:, 1])


def sensor_delay(seed, robot_offset, lat_tick, lat, enc, line, eline, obs, nu):
    """duck_fleet_sensor_delay. line [N][3][6], eline [N][3][2 nu], obs [N][O] float32 numpy, updated in place
    through int32 views; lat_tick int32 [N] is not written. Returns (IMU d_eff [N], whether the IMU columns were
    written [N], encoder d_eff [N], whether the encoder columns were written [N])."""
    n, W = obs.shape[0], 2 * nu
    assert eline.shape == (n, SLOTS, W) and eline.dtype == f32 and obs.dtype == f32 and obs.shape[1] >= ENC_COL + W
    assert np.asarray(lat).reshape(-1, LAT_SIZE).shape[0] == n
    s_eff, s_wrote = sense_delay(seed, robot_offset, lat_tick, lat, line, obs)
    lw, ow = eline.view(np.int32), obs.view(np.int32)
    p = period(lat_tick)
    d = encoder_delay(seed, robot_offset, lat_tick, enc)
    d_eff = np.minimum(d, np.minimum(p, MAX_DELAY))
    e = np.arange(n)
    lw[e, p % SLOTS] = ow[:, ENC_COL:ENC_COL + W]
    wrote = d_eff > 0
    ow[wrote, ENC_COL:ENC_COL + W] = lw[e, (p - d_eff) % SLOTS][wrote]
    return s_eff, s_wrote, d_eff, wrote
