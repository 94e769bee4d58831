#!/usr/bin/env python
"""HER with the SAC trainer — the reference's second entry point, run_scripts/her_sac_exp_script.py: the same `experiment` as
her_td3_exp_script.py, which builds her.SAC and a tanh-Gaussian policy when the variant carries `sac_params`."""
from _common import main

from her_td3_exp_script import experiment


if __name__ == "__main__":
    main(experiment, "her")
