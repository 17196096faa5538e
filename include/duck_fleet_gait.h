/* duck_fleet_gait.h -- the host descriptor of duck_fleet_gait (duck_fleet.h, which includes this file and states
 * the entry, the record and the rule). It tells the launch where the feet's sensors are and from where on a servo
 * counts as saturated; duck_fleet_desc is not touched. Filled from the compiled model by sim2sim.gait_desc. */
#ifndef DUCK_FLEET_GAIT_H_
#define DUCK_FLEET_GAIT_H_

#include "duck_fleet.h"

typedef struct duck_fleet_gait_desc {
  int foot_linvel[2];   /* sensor_adr of left_, right_foot_global_linvel inside sensordata (3 values each) */
  int foot_pos[2];      /* sensor_adr of left_, right_foot_pos (3 values each) */
  float force_sat[DUCK_FLEET_MAX_NU]; /* a period counts as force-saturated when |force| >= this; +inf: never */
  float speed_sat;      /* a period counts as speed-saturated when |joint velocity| >= this; +inf: never */
} duck_fleet_gait_desc;

#endif /* DUCK_FLEET_GAIT_H_ */
